"""The agreement of independent restarts behind the C ABI (sdpsr_meet_keys, sdpsr_agree_partitions,
sdpsr_agree_block_diagonalization, sdpsr_comm_*) against the oracle's refine! folded over the valid inputs: bit-exact.

Inputs: 37 x 37 label matrices with 6, 8, 2, 7, 5, 3, 4, 8, 2, 6, 5 classes (uniform draws, seed 7, label 0 among them, seven
entries 0 in all of them), canonical through oracle.partition_from_labels.  Their meets have 62 (R = 2), 188 (R = 3), more
than 255 (R = 5) and at most 1369 (R = 11) classes: R = 2 and 3 fit 8-bit labels, R = 5 must overflow them."""
import ctypes as C
import os
import subprocess
import sys
from functools import reduce

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 37
LEN = N * N
CLASSES = [6, 8, 2, 7, 5, 3, 4, 8, 2, 6, 5]
BAD_ARGUMENT, LABEL_OVERFLOW, BAD_STATE = 5, 4, 10
CANARY = 0xA5A5A5A55A5A5A5A


def make_inputs(oracle):
    rng = np.random.default_rng(7)
    Ms = [rng.integers(0, k + 1, size=(N, N)) for k in CLASSES]
    for M in Ms:
        M[5, :7] = 0
    return [oracle.partition_from_labels(M) for M in Ms]


@pytest.fixture(scope="module")
def inputs(oracle):
    """(the eleven partitions, {R: the oracle's meet of the first R}) -- computed once, never modified."""
    ps = make_inputs(oracle)
    meets = {R: reduce(oracle.refine, ps[:R]) for R in (2, 3, 4, 5, 11)}
    assert [p.nparts for p in ps] == CLASSES
    assert meets[2].nparts == 62 and meets[3].nparts == 188 and meets[5].nparts > 255 and meets[11].nparts <= LEN
    for m in meets.values():  # zeros remain exactly where all inputs are 0
        assert int((m.matrix == 0).sum()) >= 7
    return ps, meets


@pytest.fixture(scope="module")
def ctxs(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cs = {B: pkg.Context(device=0, seed=99, label_width=B) for B in (8, 16, 32)}
    yield cs
    for c in cs.values():
        c.close()


def flat(P, dt):
    return np.ascontiguousarray(np.asarray(P.matrix).ravel(order="F").astype(dt))


def multiplier(pkg, k):
    return pkg.parallel._slot_multiplier(k) % 2 ** 64


def keys_reference(pkg, arrays, valid, first_slot):
    acc = np.zeros(arrays[0].size, dtype=np.uint64)
    for i, a in enumerate(arrays):
        if valid is None or valid[i]:
            acc += a.astype(np.uint64) * np.uint64(multiplier(pkg, first_slot + i))  # wraps mod 2^64
    return acc


class Arrays:
    """R label arrays in one memory space, every one starting `offset_elems` elements behind a 16-byte boundary."""

    def __init__(self, arrays, mem, offset_elems=0):
        import torch
        self.mem, self.R = mem, len(arrays)
        self.dt, self.n = arrays[0].dtype, arrays[0].size
        eb = self.dt.itemsize
        self.nbytes = self.n * eb
        self.bufs, self.ptr_values = [], []
        for a in arrays:
            raw = np.frombuffer(a.tobytes(), dtype=np.uint8)
            if mem == 1:
                buf = torch.zeros(self.nbytes + 64, dtype=torch.uint8, device="cuda")
                base = buf.data_ptr()
            else:
                buf = np.zeros(self.nbytes + 64, dtype=np.uint8)
                base = buf.ctypes.data
            off = (-base) % 16 + offset_elems * eb
            if mem == 1:
                buf[off:off + self.nbytes] = torch.from_numpy(raw.copy()).cuda()
            else:
                buf[off:off + self.nbytes] = raw
            self.bufs.append((buf, off))
            self.ptr_values.append(base + off)
        if mem == 1:
            torch.cuda.synchronize()
        self.ptrs = (C.c_void_p * self.R)(*self.ptr_values)

    def get(self, i):
        buf, off = self.bufs[i]
        piece = buf[off:off + self.nbytes]
        host = piece.cpu().numpy() if self.mem == 1 else piece
        return np.frombuffer(host.tobytes(), dtype=self.dt)


def valid_arg(valid):
    return None if valid is None else (C.c_int32 * len(valid))(*valid)


def call_agree(ctx, arrs, valid=None, comm=None, dim0=-7, met0=-7):
    dim, met = C.c_int64(dim0), C.c_int32(met0)
    st = ctx._lib.sdpsr_agree_partitions(ctx._h, comm, arrs.R, C.cast(arrs.ptrs, C.c_void_p), C.cast(valid_arg(valid), C.c_void_p), arrs.n,
                                         C.byref(dim), C.byref(met), arrs.mem)
    return st, int(met.value), int(dim.value)


# ---- sdpsr_meet_keys against the NumPy formula ------------------------------------------------------------------------------
def call_meet_keys(ctx, arrs, valid, first_slot, n, key_offset_words=1):
    """keys start `key_offset_words` words behind a 16-byte boundary, canary words on both sides; returns (status, keys, intact)."""
    import torch
    total = n + 8
    if arrs.mem == 1:
        kb = torch.full((total,), CANARY - 2 ** 64, dtype=torch.int64, device="cuda")
        base = kb.data_ptr()
    else:
        kb = np.full(total, CANARY, dtype=np.uint64)
        base = kb.ctypes.data
    w0 = ((-base) % 16) // 8 + key_offset_words
    if arrs.mem == 1:
        torch.cuda.synchronize()
    st = ctx._lib.sdpsr_meet_keys(ctx._h, arrs.R, C.cast(arrs.ptrs, C.c_void_p), C.cast(valid_arg(valid), C.c_void_p), n, first_slot,
                                  C.c_void_p(base + 8 * w0), arrs.mem)
    host = (kb.cpu().numpy().view(np.uint64) if arrs.mem == 1 else kb)
    intact = bool((host[:w0] == np.uint64(CANARY)).all() and (host[w0 + n:] == np.uint64(CANARY)).all())
    return st, host[w0:w0 + n].copy(), intact


def random_labels(rng, n, dt, R):
    top = np.iinfo(dt).max
    out = []
    for _ in range(R):
        a = rng.integers(0, int(top) + 1, size=n, dtype=np.uint64).astype(dt)
        a[rng.random(n) < 0.25] = 0
        a[::97] = 0      # zero in every array: the key must be 0 there
        if n > 3:
            a[3] = top   # the largest label of the width
        out.append(a)
    return out


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_meet_keys_matches_the_formula(pkg, ctxs, bits, mem):
    """Every length at which the pass changes shape (head only, one piece less / exactly / more than a lane's 16 bytes at each
    width, head + body + tail), R = 1, 2, 5, 64, first slots across the k mod 8 and floor(k / 8) steps, masks that drop the
    first and the last restart; every array one element behind a 16-byte boundary and the keys 8 bytes behind one (head of the
    key pass, element-aligned loads); canary words around the keys."""
    ctx, dt = ctxs[bits], np.dtype({8: np.uint8, 16: np.uint16, 32: np.uint32}[bits])
    rng = np.random.default_rng(100 + bits + mem)
    combos = [(1, 0, None), (2, 6, [0, 1]), (5, 8, [1, 1, 1, 1, 0]), (64, 130, None)]
    for n in (1, 15, 16, 17, LEN):
        for R, first_slot, valid in combos:
            arrays = random_labels(rng, n, dt, R)
            arrs = Arrays(arrays, mem, offset_elems=1)
            st, keys, intact = call_meet_keys(ctx, arrs, valid, first_slot, n)
            assert st == 0, (n, R, ctx._lib.sdpsr_last_error(ctx._h))
            assert intact, (n, R)
            ref = keys_reference(pkg, arrays, valid, first_slot)
            assert np.array_equal(keys, ref), (n, R, first_slot)
            assert not keys[::97].any()
    # aligned arrays and aligned keys take the other load form and no head
    arrays = random_labels(rng, LEN, dt, 3)
    st, keys, intact = call_meet_keys(ctx, Arrays(arrays, mem, 0), None, 0, LEN, key_offset_words=0)
    assert st == 0 and intact and np.array_equal(keys, keys_reference(pkg, arrays, None, 0))


@pytest.fixture(scope="module")
def long_arrays():
    """Two arrays of 16 MB + 5 labels per width (2^22 + 5 labels at width 32), drawn once."""
    return {bits: random_labels(np.random.default_rng(5), 2 ** 22 * (32 // bits) + 5, np.dtype(dt), 2)
            for bits, dt in ((8, np.uint8), (16, np.uint16), (32, np.uint32))}


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_meet_keys_more_than_one_grid_stride_trip(pkg, ctxs, long_arrays, bits, mem):
    """16 MB per array (2^22 + 5 entries at width 32): 2^20 + 1 16-byte pieces against the grid's cap of 8 workgroups of 256 lanes
    on each of 256 CUs -- the one length here at which a lane makes more than one trip of the grid-stride loop; R = 2 arrays, one
    element off a 16-byte boundary."""
    ctx, arrays = ctxs[bits], long_arrays[bits]
    n = arrays[0].size
    st, keys, intact = call_meet_keys(ctx, Arrays(arrays, mem, offset_elems=1), None, 6, n)
    assert st == 0 and intact
    assert np.array_equal(keys, keys_reference(pkg, arrays, None, 6))


def test_meet_keys_argument_errors_leave_the_ctx_usable(pkg, ctxs):
    ctx = ctxs[32]
    arrays = random_labels(np.random.default_rng(1), 40, np.dtype(np.uint32), 2)
    arrs = Arrays(arrays, 0)
    keys = np.zeros(40, dtype=np.uint64)
    kp, lp = C.c_void_p(keys.ctypes.data), C.cast(arrs.ptrs, C.c_void_p)
    f = ctx._lib.sdpsr_meet_keys
    assert f(ctx._h, 0, lp, None, 40, 0, kp, 0) == BAD_ARGUMENT
    assert f(ctx._h, 65, lp, None, 40, 0, kp, 0) == BAD_ARGUMENT
    assert f(ctx._h, 2, None, None, 40, 0, kp, 0) == BAD_ARGUMENT
    assert f(ctx._h, 2, lp, None, 40, 0, None, 0) == BAD_ARGUMENT
    assert f(ctx._h, 2, lp, None, 0, 0, kp, 0) == BAD_ARGUMENT
    assert f(ctx._h, 2, lp, None, 40, -1, kp, 0) == BAD_ARGUMENT
    assert f(ctx._h, 2, C.cast((C.c_void_p * 2)(arrs.ptr_values[0], None), C.c_void_p), None, 40, 0, kp, 0) == BAD_ARGUMENT
    assert f(ctx._h, 2, lp, None, 40, 0, kp, 0) == 0
    assert np.array_equal(keys, keys_reference(pkg, arrays, None, 0))


def test_two_ranks_emulated_on_one_gpu(pkg, ctxs, inputs):
    """What two ranks of two restarts compute: keys for the slots 0, 1 and 2, 3 from two calls, added with wrap-around (the
    all-reduce), relabelled by sdpsr_partition_from_u64 -- the oracle's meet of the four."""
    ps, meets = inputs
    for bits in (16, 32):
        ctx, dt = ctxs[bits], ctxs[bits].label_dtype
        arrays = [flat(p, dt) for p in ps[:4]]
        k01 = pkg.meet_keys(arrays[:2], first_slot=0, ctx=ctx)
        k23 = pkg.meet_keys(arrays[2:], first_slot=2, ctx=ctx)
        total = k01 + k23  # uint64: wraps
        assert np.array_equal(total, keys_reference(pkg, arrays, None, 0))
        out, n = np.zeros(LEN, dtype=dt), C.c_int64(0)
        ctx.check(ctx._lib.sdpsr_partition_from_u64(ctx._h, LEN, C.c_void_p(total.ctypes.data), C.c_void_p(out.ctypes.data), C.byref(n), 0))
        assert n.value == meets[4].nparts
        assert np.array_equal(out, flat(meets[4], dt))


# ---- sdpsr_agree_partitions, comm = NULL ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_agree_partitions_meet(ctxs, inputs, bits, mem):
    """Disagreeing restarts: every array ends as the oracle's meet, met = 1, dim_out its class count -- R = 2, 3 at every
    width, R = 11 where 1369 classes fit; arrays one element off a 16-byte boundary."""
    ps, meets = inputs
    ctx, dt = ctxs[bits], ctxs[bits].label_dtype
    for R in (2, 3, 11):
        if meets[R].nparts > np.iinfo(dt).max:
            assert bits == 8 and R == 11
            continue
        arrs = Arrays([flat(p, dt) for p in ps[:R]], mem, offset_elems=1)
        st, met, dim = call_agree(ctx, arrs)
        assert (st, met, dim) == (0, 1, meets[R].nparts), ctx._lib.sdpsr_last_error(ctx._h)
        want = flat(meets[R], dt)
        for i in range(R):
            assert np.array_equal(arrs.get(i), want), (R, i)


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_agree_partitions_agreement_coarsened_and_invalid(oracle, ctxs, inputs, bits, mem):
    ps, meets = inputs
    ctx, dt = ctxs[bits], ctxs[bits].label_dtype
    fine = flat(meets[3], dt)  # 188 classes
    # R copies of one partition: nothing is written, dim_out and the arrays stay
    arrs = Arrays([fine.copy() for _ in range(4)], mem)
    assert call_agree(ctx, arrs) == (0, 0, -7)
    assert all(np.array_equal(arrs.get(i), fine) for i in range(4))
    # a coarsened copy (two classes merged -- a split one restart's draws missed) among fine ones: everybody ends fine
    M = np.asarray(meets[3].matrix).copy()
    M[M == 17] = 5
    coarse = oracle.partition_from_labels(M)
    assert coarse.nparts == 187
    for pos in (0, 2):
        parts = [fine.copy(), fine.copy(), fine.copy()]
        parts[pos] = flat(coarse, dt)
        arrs = Arrays(parts, mem)
        assert call_agree(ctx, arrs) == (0, 1, 188)
        assert all(np.array_equal(arrs.get(i), fine) for i in range(3))
    # an invalid restart full of garbage above d: it does not influence the result and holds it afterwards
    rng = np.random.default_rng(3)
    garbage = rng.integers(200, 256, size=LEN).astype(dt)
    want = flat(meets[2], dt)
    for pos in (0, 2):
        parts = [flat(ps[0], dt), flat(ps[1], dt)]
        parts.insert(pos, garbage.copy())
        valid = [1, 1, 1]
        valid[pos] = 0
        arrs = Arrays(parts, mem)
        assert call_agree(ctx, arrs, valid) == (0, 1, 62)
        assert all(np.array_equal(arrs.get(i), want) for i in range(3))
    # an invalid restart beside agreeing ones: a meet all the same -- it has to receive the partition
    arrs = Arrays([fine.copy(), garbage.copy(), fine.copy()], mem)
    assert call_agree(ctx, arrs, [1, 0, 1]) == (0, 1, 188)
    assert all(np.array_equal(arrs.get(i), fine) for i in range(3))
    # nothing valid
    arrs = Arrays([fine.copy(), garbage.copy()], mem)
    st, met, dim = call_agree(ctx, arrs, [0, 0])
    assert st == BAD_STATE and (met, dim) == (-7, -7)
    assert np.array_equal(arrs.get(0), fine) and np.array_equal(arrs.get(1), garbage)
    assert call_agree(ctx, arrs, [1, 0]) == (0, 1, 188)  # the ctx stays usable


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
def test_agree_partitions_overflow_at_width_8(ctxs, inputs, mem):
    """R = 5: the meet has more than 255 classes -- SDPSR_LABEL_OVERFLOW with the count in dim_out and every array untouched."""
    ps, meets = inputs
    ctx = ctxs[8]
    parts = [flat(p, np.uint8) for p in ps[:5]]
    arrs = Arrays(parts, mem)
    st, met, dim = call_agree(ctx, arrs)
    assert st == LABEL_OVERFLOW and dim == meets[5].nparts and met == -7
    assert all(np.array_equal(arrs.get(i), parts[i]) for i in range(5))
    assert call_agree(ctx, Arrays(parts[:2], mem)) == (0, 1, 62)


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_agree_partitions_transfer_bytes(ctxs, inputs, bits):
    """Host arrays: the valid ones are uploaded once, all R come back only after a meet; 16 bytes of checksum per restart."""
    ps, meets = inputs
    ctx, dt = ctxs[bits], ctxs[bits].label_dtype
    nb = LEN * dt.itemsize
    h0, d0 = ctx.transfer_bytes()
    assert call_agree(ctx, Arrays([flat(ps[0], dt), flat(ps[1], dt), flat(ps[2], dt)], 0), [1, 1, 0]) == (0, 1, 62)
    h1, d1 = ctx.transfer_bytes()
    assert (h1 - h0, d1 - d0) == (2 * nb, 3 * nb + 3 * 16)
    assert call_agree(ctx, Arrays([flat(meets[2], dt)] * 3, 0)) == (0, 0, -7)
    h2, d2 = ctx.transfer_bytes()
    assert (h2 - h1, d2 - d1) == (3 * nb, 3 * 16)
    dev = Arrays([flat(ps[0], dt), flat(ps[1], dt)], 1)
    assert call_agree(ctx, dev) == (0, 1, 62)
    h3, d3 = ctx.transfer_bytes()
    assert (h3 - h2, d3 - d2) == (0, 2 * 16)


def test_agree_partitions_argument_errors_leave_the_ctx_usable(ctxs, inputs):
    ps, meets = inputs
    ctx = ctxs[16]
    parts = [flat(ps[0], np.uint16), flat(ps[1], np.uint16)]
    arrs = Arrays(parts, 0)
    lp = C.cast(arrs.ptrs, C.c_void_p)
    dim, met = C.c_int64(-7), C.c_int32(-7)
    f = ctx._lib.sdpsr_agree_partitions
    assert f(ctx._h, None, 0, lp, None, LEN, C.byref(dim), C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 65, lp, None, LEN, C.byref(dim), C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 2, None, None, LEN, C.byref(dim), C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 2, C.cast((C.c_void_p * 2)(arrs.ptr_values[0], None), C.c_void_p), None, LEN, C.byref(dim), C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 2, lp, None, 0, C.byref(dim), C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 2, lp, None, 2 ** 32, C.byref(dim), C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 2, lp, None, LEN, None, C.byref(met), 0) == BAD_ARGUMENT
    assert f(ctx._h, None, 2, lp, None, LEN, C.byref(dim), None, 0) == BAD_ARGUMENT
    assert (dim.value, met.value) == (-7, -7)
    assert all(np.array_equal(arrs.get(i), parts[i]) for i in range(2))
    dev = Arrays(parts, 1, offset_elems=0)
    odd = C.cast((C.c_void_p * 2)(dev.ptr_values[0] + 1, dev.ptr_values[1]), C.c_void_p)  # not aligned to its element
    assert f(ctx._h, None, 2, odd, None, LEN - 1, C.byref(dim), C.byref(met), 1) == BAD_ARGUMENT
    assert call_agree(ctx, arrs) == (0, 1, 62)
    assert np.array_equal(arrs.get(1), flat(meets[2], np.uint16))


def test_agree_block_diagonalization_alone(pkg, ctxs):
    ctx = ctxs[32]
    assert pkg.agree_block_diagonalization(0, [3, 1, 2], ctx=ctx) == (0, [3, 1, 2])
    assert pkg.agree_block_diagonalization(3, [3, 1, 2], ctx=ctx) == (-1, None)
    assert pkg.agree_block_diagonalization(2, None, ctx=ctx) == (-1, None)
    sizes = np.array([4, 5, 6], dtype=np.int32)
    out = np.full(2, -1, dtype=np.int32)
    w, nb = C.c_int32(-9), C.c_int32(-9)
    st = ctx._lib.sdpsr_agree_block_diagonalization(ctx._h, None, 0, 3, C.c_void_p(sizes.ctypes.data), C.byref(w), C.byref(nb),
                                                    C.c_void_p(out.ctypes.data), 2)
    assert st == BAD_ARGUMENT and (w.value, nb.value) == (0, 3) and out.tolist() == [-1, -1]
    assert pkg.agree_block_diagonalization(0, [7], ctx=ctx) == (0, [7])


# ---- Python level -----------------------------------------------------------------------------------------------------------
def test_python_agree_partitions_on_a_reduce_batch(pkg, problems, oracle):
    """Problem.reduce_batch(restarts=2) of ER(3), one result coarsened by hand: agree_partitions over the restarts with a
    status in {0, 2, 3} returns the uncoarsened partition -- on Partitions and on CUDA tensors, in place."""
    import torch
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(3))
    with pkg.Context(device=0, seed=11) as ctx:
        with pkg.Problem(Cv, A, b, ctx=ctx) as prob:
            res = prob.reduce_batch(restarts=2, seeds=[1, 2])
        valid = [r["status"] in pkg.agree.VALID_STATUSES for r in res]
        assert all(valid)
        P0, P1 = res[0]["P"], res[1]["P"]
        assert P0 == P1
        met, P = pkg.agree_partitions([P0, P1], valid=valid, ctx=ctx)
        assert met is False and P == P0
        M = np.asarray(P1.matrix).astype(np.int64)
        M[M == P1.nparts] = 1  # merge the last class into the first
        co = oracle.partition_from_labels(M)
        coarse = pkg.Partition(co.nparts, co.matrix.astype(np.uint32))
        assert coarse.nparts == P0.nparts - 1
        met, P = pkg.agree_partitions([coarse, P0], valid=valid, ctx=ctx)
        assert met is True and P == P0 and P.nparts == P0.nparts
        f0 = np.ascontiguousarray(np.asarray(P0.matrix).ravel(order="F").astype(np.uint32))
        t_fine = torch.from_numpy(f0.view(np.int32).copy()).cuda()
        t_coarse = torch.from_numpy(np.asarray(coarse.matrix).ravel(order="F").astype(np.uint32).view(np.int32).copy()).cuda()
        met, d = pkg.agree_partitions([t_fine, t_coarse], ctx=ctx)
        assert met is True and d == P0.nparts
        assert np.array_equal(t_coarse.cpu().numpy().view(np.uint32), f0) and np.array_equal(t_fine.cpu().numpy().view(np.uint32), f0)
        met, d = pkg.agree_partitions([t_fine, t_coarse], ctx=ctx)
        assert met is False and d == P0.nparts


# ---- one RCCL rank, in a process of its own ----------------------------------------------------------------------------------
RCCL_CHILD = r"""
import os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "oracle"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import ctypes as C
import numpy as np, torch
import sdpsr_oracle as O
from functools import reduce
from __graft_entry__ import load_package
import test_gpu_agree as T
pkg = load_package()
ps = T.make_inputs(O)
meet = reduce(O.refine, ps[:2])
dev = torch.device("cuda:0")
def cuda(p):
    return torch.from_numpy(T.flat(p, np.uint32).view(np.int32).copy()).to(dev)
ctx = pkg.Context(device=0, seed=5)
alone = [cuda(ps[0]), cuda(ps[1])]
assert pkg.agree_partitions(alone, ctx=ctx) == (True, meet.nparts)
comm = pkg.Comm(1, 0, pkg.Comm.unique_id(), ctx=ctx)
assert (comm.rank, comm.world) == (0, 1)
pair = [cuda(ps[0]), cuda(ps[1])]
assert pkg.agree_partitions(pair, comm=comm) == (True, meet.nparts)
want = T.flat(meet, np.uint32)
for t, a in zip(pair, alone):
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want) and bool((t == a).all())
same = [cuda(meet), cuda(meet)]
assert pkg.agree_partitions(same, comm=comm) == (False, meet.nparts)
assert all(np.array_equal(t.cpu().numpy().view(np.uint32), want) for t in same)
host = [T.flat(ps[0], np.uint32), T.flat(ps[1], np.uint32)]
met, P = pkg.agree_partitions(host, comm=comm)
assert met and P.nparts == meet.nparts and np.array_equal(host[0], want) and np.array_equal(host[1], want)
assert pkg.agree_block_diagonalization(0, [2, 2, 3, 1], comm=comm) == (0, [2, 2, 3, 1])
assert pkg.agree_block_diagonalization(3, [2, 2], comm=comm) == (-1, None)
buf = torch.arange(1000, dtype=torch.float64, device=dev)
keep = buf.clone()
assert comm.broadcast(buf, root=0) is buf and bool((buf == keep).all())
hb = np.arange(77, dtype=np.float64)
comm.broadcast(hb, root=0)
assert np.array_equal(hb, np.arange(77, dtype=np.float64))
st = ctx._lib.sdpsr_comm_broadcast(ctx._h, comm._h, C.c_void_p(buf.data_ptr()), 8, 1, 1)   # a root outside the world
assert st == 5, st
comm.close()
ctx.close()
print("RCCL_AGREE_ONE_RANK_OK")
"""


def test_rccl_one_rank_agreement_in_a_child_process():
    """RCCL refuses two ranks on one device and the test machines expose one GPU: what can be shown is that the communicator
    path runs -- unique id, sdpsr_comm_create(world = 1), the all-gather of the records, the SUM all-reduce of the keys, the
    broadcasts -- and returns what comm = NULL and the oracle give.  In a fresh child process with a time-out; a library that
    cannot be opened is a failure, not a skip."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["NCCL_SOCKET_IFNAME"] = "lo"
    out = subprocess.run([sys.executable, "-c", RCCL_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RCCL_AGREE_ONE_RANK_OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
