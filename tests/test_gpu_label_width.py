"""Label arrays in the reference's own widths (Partition{T}, T = UInt8 / UInt16; src/partitions.jl:6-11,84) across the ABI:
the conversion kernels against ``astype`` at every length and alignment at which they take another path, every governed
entry point at widths 8 and 16 against the same call at width 32, device-resident narrow arrays, the bytes that cross, the
overflow contract (count set, labels untouched) and the setter."""
import ctypes as C
import pathlib

import numpy as np
import pytest

import label_width_ref as ref

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, LABEL_OVERFLOW, BAD_ARGUMENT = 0, 4, 5
HOST, DEVICE = 0, 1
RTOL = float(np.sqrt(np.finfo(np.float64).eps))
GUARD = 32  # guard elements on each side of an output
DIRECTIONS = [(32, 16), (32, 8), (16, 32), (8, 32)]
LENGTHS = [1, 7, 8, 15, 16, 17, 31, 4095, 4096, 4097, 65539]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _problem(problems, name):
    if name.startswith("er"):
        return problems.theta_prime_problem(problems.er_graph_adjacency(int(name[2:])))
    fa, fb = problems.read_qapdata(ROOT / "tests" / "golden" / "esc16j.dat")
    return problems.qap_problem(fa, fb)


@pytest.fixture(scope="module")
def setups(pkg, problems):
    """name -> host Setup (n, CL, X0L, U) of the three problems, computed once."""
    return {name: pkg.admissible_setup(*_problem(problems, name)) for name in ("er5", "er7", "esc16j")}


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with pkg.Context(seed=77) as c:
        yield c


# ------------------------------------------------------------------ 1. the conversion kernels
def _device_bytes(torch, nbytes):
    return torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")


def _convert_device(torch, ctx, src, in_bits, out_bits, off_in, off_out):
    """src (numpy, in_bits) converted on the device between two sub-arrays that start off_in / off_out ELEMENTS into their
    allocations; returns (status, out array, guards unchanged?)."""
    ib, ob = in_bits // 8, out_bits // 8
    n = src.size
    tin = _device_bytes(torch, (n + off_in) * ib)
    tin[off_in * ib:(off_in + n) * ib] = torch.from_numpy(src.view(np.uint8).copy()).cuda()
    tout = torch.full(((n + off_out + 2 * GUARD) * ob + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = (GUARD + off_out) * ob
    torch.cuda.synchronize()
    st = ctx._lib.sdpsr_labels_convert(ctx._h, n, C.c_void_p(tin.data_ptr() + off_in * ib), in_bits, C.c_void_p(tout.data_ptr() + lo), out_bits, DEVICE)
    raw = tout.cpu().numpy()
    out = raw[lo:lo + n * ob].copy().view(ref.DTYPES[out_bits])
    guards_ok = bool((raw[:lo] == 0xA5).all() and (raw[lo + n * ob:] == 0xA5).all())
    return st, out, guards_ok


def _convert_host(ctx, src, in_bits, out_bits):
    n = src.size
    buf = np.full(n + 2 * GUARD, 0xA5A5A5A5 & ref.typemax(out_bits), dtype=ref.DTYPES[out_bits])
    out = buf[GUARD:GUARD + n]
    st = ctx._lib.sdpsr_labels_convert(ctx._h, n, _vp(src), in_bits, _vp(out), out_bits, HOST)
    sentinel = buf[0]
    guards_ok = bool((buf[:GUARD] == sentinel).all() and (buf[GUARD + n:] == sentinel).all())
    return st, out.copy(), guards_ok


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("in_bits,out_bits", DIRECTIONS)
def test_convert_equals_astype_at_every_length_and_alignment(ctx, in_bits, out_bits, mem):
    import torch
    fit = min(in_bits, out_bits)
    for len_ in LENGTHS:
        src = ref.random_labels(len_, fit, seed=1000 * in_bits + len_).astype(ref.DTYPES[in_bits])
        expect = ref.convert_reference(src, out_bits)
        if mem == "host":
            st, out, guards_ok = _convert_host(ctx, src, in_bits, out_bits)
            assert st == OK and guards_ok and np.array_equal(out, expect), (len_,)
            continue
        # sub-arrays 0, 1 and 3 elements into an allocation: input, output or both off the 16-byte boundary
        for off_in, off_out in ((0, 0), (1, 0), (0, 1), (3, 0), (0, 3), (1, 3), (3, 3)):
            st, out, guards_ok = _convert_device(torch, ctx, src, in_bits, out_bits, off_in, off_out)
            assert st == OK and guards_ok, (len_, off_in, off_out)
            assert np.array_equal(out, expect), (len_, off_in, off_out)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("out_bits", [16, 8])
def test_convert_reports_a_single_value_that_does_not_fit(ctx, out_bits, mem):
    import torch
    for len_ in (1, 17, 4097):
        for pos in sorted({0, len_ // 2, len_ - 1}):
            src = ref.random_labels(len_, out_bits, seed=len_ + pos).astype(np.uint32)
            src[pos] = ref.typemax(out_bits) + 1
            with pytest.raises(ref.Inexact):
                ref.convert_reference(src, out_bits)
            if mem == "host":
                st, _, guards_ok = _convert_host(ctx, src, 32, out_bits)
            else:
                st, _, guards_ok = _convert_device(torch, ctx, src, 32, out_bits, 1, 1)
            assert st == LABEL_OVERFLOW and guards_ok, (len_, pos)
            # the ctx stays usable
            good = src.copy()
            good[pos] = ref.typemax(out_bits)
            st, out, _ = _convert_host(ctx, good, 32, out_bits)
            assert st == OK and np.array_equal(out, ref.convert_reference(good, out_bits))


def test_convert_rejects_bad_arguments(ctx):
    lib = ctx._lib
    a, b = np.arange(8, dtype=np.uint32), np.zeros(8, dtype=np.uint16)
    for in_bits, out_bits in ((12, 16), (32, 12), (64, 32), (32, 0)):
        assert lib.sdpsr_labels_convert(ctx._h, 8, _vp(a), in_bits, _vp(b), out_bits, HOST) == BAD_ARGUMENT
    assert lib.sdpsr_labels_convert(ctx._h, 8, None, 32, _vp(b), 16, HOST) == BAD_ARGUMENT
    assert lib.sdpsr_labels_convert(ctx._h, 8, _vp(a), 32, None, 16, HOST) == BAD_ARGUMENT
    assert lib.sdpsr_labels_convert(ctx._h, -1, _vp(a), 32, _vp(b), 16, HOST) == BAD_ARGUMENT
    assert np.array_equal(b, np.zeros(8, dtype=np.uint16))
    assert lib.sdpsr_labels_convert(ctx._h, 8, _vp(a), 32, _vp(b), 16, HOST) == OK and np.array_equal(b, a)


def test_labels_convert_of_the_python_mirror(pkg, ctx):
    import torch
    a = ref.random_labels(1000, 8, seed=3).astype(np.uint32)
    assert np.array_equal(pkg.labels_convert(a, 8, ctx=ctx), a.astype(np.uint8))
    t = torch.from_numpy(a.astype(np.uint8)).cuda()
    w = pkg.labels_convert(t, 32, ctx=ctx)
    assert w.dtype == torch.int32 and np.array_equal(w.cpu().numpy().view(np.uint32), a)
    a[5] = 256
    with pytest.raises(pkg.LabelOverflow):
        pkg.labels_convert(a, 8, ctx=ctx)


# ------------------------------------------------------------------ 2. every governed entry, widths 8 and 16 against 32
def _pair(pkg, bits, seed, **kw):
    """Two contexts with the same seed: width 32 and width ``bits``."""
    return pkg.Context(seed=seed, **kw), pkg.Context(seed=seed, label_width=bits, **kw)


def _same_partition(Pw, Pn, bits):
    assert Pn.matrix.dtype == ref.DTYPES[bits] and Pw.matrix.dtype == np.uint32
    assert Pn.nparts == Pw.nparts
    assert np.array_equal(Pn.matrix, ref.convert_reference(Pw.matrix, bits))


def _same_images(a, b):
    assert a.blkSizes == b.blkSizes
    for ra, rb in zip(a.blks, b.blks):
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)  # bit-equal: same labels, same draws
    for x, y in zip(a.Q_hat, b.Q_hat):
        assert np.array_equal(x, y)


def _narrow_twin(pkg, Pw, bits, fn_narrow):
    """The narrow context's result of a call whose width-32 result is the partition ``Pw``: the same partition, or -- when it
    has more classes than the width holds -- the reference's InexactError."""
    if Pw.nparts > ref.typemax(bits):
        with pytest.raises(pkg.LabelOverflow):
            fn_narrow()
        return
    _same_partition(Pw, fn_narrow(), bits)


def _parity_labels(n):
    i = np.arange(n)
    return (1 + (i[:, None] % 2) + 2 * (i[None, :] % 2)).astype(np.uint32)


def _outcome(fn):
    """(result, None) or (None, exception class) of the randomized decompositions ("try again" in the reference)."""
    try:
        return fn(), None
    except Exception as e:  # noqa: BLE001
        return None, type(e)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", ["er5", "er7", "esc16j"])
def test_primitives_at_narrow_width_equal_width_32(pkg, problems, golden, name, bits):
    Lg = golden[f"{name}_P"]
    d = int(Lg.max())
    n = Lg.shape[0]
    rng = np.random.default_rng(5)
    values = rng.random(d)
    Cv, A, b = _problem(problems, name)
    A = np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)
    cw, cn = _pair(pkg, bits, seed=11)
    with cw, cn:
        assert cw.label_width == 32 and cn.label_width == bits and cn.label_dtype == ref.DTYPES[bits]
        # Partition{T}(M): float, 32-bit integer and 64-bit integer entries
        Mf = np.concatenate([[0.0], values])[Lg]
        Mi = (Lg.astype(np.int64) * 7919) % 100003
        Mi[Lg == 0] = 0
        Ml = Mi + (Lg.astype(np.int64) << 33)
        for M in (Mf, Mi, Ml):
            Pw, Pn = pkg.Partition.from_matrix(M, ctx=cw), pkg.Partition.from_matrix(M, ctx=cn)
            _same_partition(Pw, Pn, bits)
        assert np.array_equal(pkg.Partition.from_matrix(Mf, ctx=cw).matrix, Lg)  # (golden: labels by first occurrence)
        Pw, Pn = pkg.Partition(d, Lg.copy()), pkg.Partition(d, Lg.astype(ref.DTYPES[bits]))
        # == as the 128-bit checksum
        assert pkg.partition_checksum(Pw, ctx=cw) == pkg.partition_checksum(Pn, ctx=cn)
        # fill!, randomize!: bit-equal
        assert np.array_equal(pkg.fill(Pw, values, ctx=cw), pkg.fill(Pn, values, ctx=cn))
        assert np.array_equal(pkg.randomize(Pw, ctx=cw), pkg.randomize(Pn, ctx=cn))
        # refine!(P, P'): P' = four classes by the parities of the row and the column (it splits classes of P)
        coarse = _parity_labels(n)
        Qw, Qn = pkg.Partition.from_matrix(coarse, ctx=cw), pkg.Partition.from_matrix(coarse, ctx=cn)
        Rw = pkg.refine(pkg.Partition(d, Lg.copy()), Qw, ctx=cw)
        assert Rw.nparts > d
        _narrow_twin(pkg, Rw, bits, lambda: pkg.refine(pkg.Partition(d, Lg.astype(ref.DTYPES[bits])), Qn, ctx=cn))
        # desymmetrize
        _narrow_twin(pkg, pkg.desymmetrize(Pw, ctx=cw), bits, lambda: pkg.desymmetrize(Pn, ctx=cn))
        # A * PMat, dense and CSR: bit-equal
        if (d + 1) * min(A.shape[0], 64) * 8 <= 60 * 1024:
            assert np.array_equal(pkg.reduce_constraints(Pw, A, ctx=cw), pkg.reduce_constraints(Pn, A, ctx=cn))
        assert np.array_equal(pkg.reduce_constraints_csr(Pw, A, ctx=cw), pkg.reduce_constraints_csr(Pn, A, ctx=cn))


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", ["er5", "er7", "esc16j"])
def test_admissible_subspace_routes_at_narrow_width(pkg, problems, golden, setups, name, bits):
    Cv, A, b = _problem(problems, name)
    Lg = golden[f"{name}_P"]
    routes = [("host setup", {"setup": setups[name]}), ("device setup", {}), ("csr setup", {"csr_setup": True})]
    for what, kw in routes:
        cw, cn = _pair(pkg, bits, seed=21)
        with cw, cn:
            Pw = pkg.admissible_subspace(Cv, A, b, ctx=cw, **kw)
            Pn = pkg.admissible_subspace(Cv, A, b, ctx=cn, **kw)
            _same_partition(Pw, Pn, bits)
            assert (Pw.iterations, Pw.dims) == (Pn.iterations, Pn.dims), what
            assert np.array_equal(Pw.matrix, Lg), what
            assert pkg.partition_checksum(Pw, ctx=cw) == pkg.partition_checksum(Pn, ctx=cn)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", ["er5", "er7", "esc16j"])
def test_block_diagonalize_at_narrow_width(pkg, golden, name, bits):
    Lg = golden[f"{name}_P"]
    d = int(Lg.max())
    done = False
    for seed in (31, 32, 33, 34):
        cw, cn = _pair(pkg, bits, seed=seed)
        with cw, cn:
            rw, ew = _outcome(lambda: pkg.blockDiagonalize(pkg.Partition(d, Lg.copy()), ctx=cw))
            rn, en = _outcome(lambda: pkg.blockDiagonalize(pkg.Partition(d, Lg.astype(ref.DTYPES[bits])), ctx=cn))
            assert ew == en, (seed, ew, en)
            if ew is None:
                _same_images(rw, rn)
                assert sorted(rw.blkSizes) == list(golden[f"{name}_blk"])
                done = True
                break
            assert ew in (pkg.NumericalInconsistency, pkg.DimensionMismatch)
    assert done
    # the complex twin: same outcome at both widths, same desymmetrized partition and images when it succeeds; a desymmetrized
    # partition (canonical: it does not depend on the draws) with more classes than the width holds is the InexactError
    with pkg.Context(seed=40) as c0:
        desym_dim = pkg.desymmetrize(pkg.Partition(d, Lg.copy()), ctx=c0).nparts
    for seed in (41, 42):
        cw, cn = _pair(pkg, bits, seed=seed)
        with cw, cn:
            rw, ew = _outcome(lambda: pkg.blockDiagonalize(pkg.Partition(d, Lg.copy()), complex=True, ctx=cw))
            rn, en = _outcome(lambda: pkg.blockDiagonalize(pkg.Partition(d, Lg.astype(ref.DTYPES[bits])), complex=True, ctx=cn))
            if desym_dim > ref.typemax(bits):
                assert en is pkg.LabelOverflow
                continue
            assert ew == en, (seed, ew, en)
            if ew is None:
                _same_images(rw, rn)
                _same_partition(rw.partition, rn.partition, bits)


@pytest.mark.parametrize("bits", [8, 16])
def test_complex_block_diagonalize_of_a_cyclic_scheme_at_narrow_width(pkg, bits):
    n = 63
    i = np.arange(n)
    Lm = ((i[None, :] - i[:, None]) % n + 1).astype(np.uint32)
    cw, cn = _pair(pkg, bits, seed=9)
    with cw, cn:
        rw = pkg.blockDiagonalize(pkg.Partition(n, Lm.copy()), complex=True, ctx=cw)
        rn = pkg.blockDiagonalize(pkg.Partition(n, Lm.astype(ref.DTYPES[bits])), complex=True, ctx=cn)
        assert rw.blkSizes == [1] * n
        _same_images(rw, rn)
        _same_partition(rw.partition, rn.partition, bits)


@pytest.mark.parametrize("bits", [8, 16])
def test_eigen_decomposition_at_narrow_width(pkg, golden, bits):
    L64 = golden["numerical_issues_P"]
    assert L64.shape == (64, 64)
    d = int(L64.max())
    cw, cn = _pair(pkg, bits, seed=51)
    with cw, cn:
        Pw, Pn = pkg.Partition(d, L64.copy()), pkg.Partition(d, L64.astype(ref.DTYPES[bits]))
        assert pkg.eigen_decomposition(Pw, atol=1e-7, ctx=cw) == pkg.eigen_decomposition(Pn, atol=1e-7, ctx=cn)
        bw = pkg.eigen_decomposition_batched(Pw, 64, atol=1e-7, ctx=cw, raise_on_failure=False)
        bn = pkg.eigen_decomposition_batched(Pn, 64, atol=1e-7, ctx=cn, raise_on_failure=False)
        for x, y in zip(bw, bn):
            assert np.array_equal(x, y)


def _jordan_reduce(ctx, setup, P, mem=HOST, args=None, images=True):
    """sdpsr_jordan_reduce, sizes first and the images through sdpsr_block_images; returns a dict."""
    lib = ctx._lib
    n, CL, X0L, U = setup
    r = U.shape[1]
    if args is None:
        Uf = np.asfortranarray(U)
        args = [_vp(CL), _vp(X0L), _vp(Uf) if r else None]
    dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    if setup.hint:
        lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    pP = P if isinstance(P, C.c_void_p) or P is None else _vp(P)
    st = lib.sdpsr_jordan_reduce(ctx._h, n, *args, r, RTOL, RTOL, pP, C.byref(dd), C.byref(it), C.byref(nb), C.byref(ssq), C.byref(ss),
                                 None, 0, None, 0, None, mem)
    out = {"status": st, "dim": dd.value, "iterations": it.value, "nblocks": nb.value, "sum_sq": ssq.value, "sum_s": ss.value}
    if st == OK and images:
        sizes = np.zeros(nb.value, dtype=np.int32)
        ctx.check(lib.sdpsr_block_sizes(ctx._h, _vp(sizes)))
        blks = np.zeros(dd.value * ssq.value)
        ctx.check(lib.sdpsr_block_images(ctx._h, _vp(blks), None, None, HOST))
        out["sizes"], out["blks"] = sizes, blks
    return out


def _same_reduction(a, b):
    for k in ("status", "dim", "iterations", "nblocks", "sum_sq", "sum_s"):
        assert a[k] == b[k], (k, a[k], b[k])
    if a["status"] == OK:
        assert np.array_equal(a["sizes"], b["sizes"]) and np.array_equal(a["blks"], b["blks"])


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", ["er5", "er7", "esc16j"])
def test_jordan_reduce_and_batch_at_narrow_width(pkg, golden, setups, name, bits):
    setup = setups[name]
    n = setup[0]
    Lg = golden[f"{name}_P"]
    cw, cn = _pair(pkg, bits, seed=61)
    with cw, cn:
        Pw, Pn = np.zeros(n * n, dtype=np.uint32), np.zeros(n * n, dtype=ref.DTYPES[bits])
        rw, rn = _jordan_reduce(cw, setup, Pw), _jordan_reduce(cn, setup, Pn)
        assert rw["status"] in (0, 2, 3)
        _same_reduction(rw, rn)
        assert np.array_equal(Pw.reshape(n, n, order="F"), Lg) and np.array_equal(Pn, ref.convert_reference(Pw, bits))
        # sdpsr_jordan_reduce_batch, R = 2, host arrays
        R = 2
        res = []
        for c, dt in ((cw, np.uint32), (cn, ref.DTYPES[bits])):
            lib = c._lib
            _, CL, X0L, U = setup
            Uf = np.asfortranarray(U)
            Ps = [np.zeros(n * n, dtype=dt) for _ in range(R)]
            pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
            seeds = (C.c_uint64 * R)(5, 6)
            dd, it, nb, ssq, ss, st = (C.c_int64 * R)(), (C.c_int32 * R)(), (C.c_int32 * R)(), (C.c_int64 * R)(), (C.c_int64 * R)(), (C.c_int32 * R)()
            if setup.hint:
                lib.sdpsr_hint_symmetric_basis(c._h, setup.hint)
            lib.sdpsr_jordan_reduce_batch(c._h, R, C.cast(seeds, C.c_void_p), n, _vp(CL), _vp(X0L), _vp(Uf) if U.shape[1] else None, U.shape[1], RTOL, RTOL,
                                          C.cast(pP, C.c_void_p), dd, it, nb, ssq, ss, None, None, st, HOST)
            res.append((Ps, list(dd), list(it), list(nb), list(ssq), list(ss), list(st)))
        assert res[0][1:] == res[1][1:]
        for i in range(R):
            assert res[0][6][i] in (0, 2, 3)
            assert np.array_equal(res[0][0][i].reshape(n, n, order="F"), Lg)
            assert np.array_equal(res[1][0][i], ref.convert_reference(res[0][0][i], bits))
        # the problem handle: reduce and reduce_batch
        with pkg.Problem(setup=setup, ctx=cw) as pw, pkg.Problem(setup=setup, ctx=cn) as pn:
            for fw, fn in ((lambda: [pw.reduce_batch(1, seeds=[7])[0]], lambda: [pn.reduce_batch(1, seeds=[7])[0]]),
                           (lambda: pw.reduce_batch(2, seeds=[8, 9]), lambda: pn.reduce_batch(2, seeds=[8, 9]))):
                for xw, xn in zip(fw(), fn()):
                    for k in ("status", "iterations", "nblocks", "sum_sq", "sum_s"):
                        assert xw[k] == xn[k]
                    assert xw["status"] in (0, 2, 3)
                    _same_partition(xw["P"], xn["P"], bits)
                    assert np.array_equal(xw["P"].matrix, Lg)
                    if xw["status"] == 0:
                        assert np.array_equal(xw["blks"], xn["blks"])


def test_problem_reduce_entry_at_width_16(pkg, golden, setups):
    """sdpsr_problem_reduce itself (the Python mirror's Problem.reduce is a one-restart batch): same counts, labels and
    images as at width 32."""
    setup = setups["esc16j"]
    n = setup[0]
    Lg = golden["esc16j_P"]
    d = int(Lg.max())
    got = []
    for width in (32, 16):
        with pkg.Context(seed=63, label_width=width) as c, pkg.Problem(setup=setup, ctx=c) as prob:
            lib = c._lib
            P = np.zeros(n * n, dtype=ref.DTYPES[width])
            dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
            blks = np.zeros(d * d * 4)  # capacity for the images: d * sum_sq with sum_sq = 255 < 4 d
            st = lib.sdpsr_problem_reduce(c._h, prob._h, RTOL, RTOL, _vp(P), C.byref(dd), C.byref(it), C.byref(nb), C.byref(ssq), C.byref(ss),
                                          _vp(blks), blks.size, None, 0, None, HOST)
            assert st in (0, 2, 3)
            got.append((st, dd.value, it.value, nb.value, ssq.value, ss.value, P, blks))
    assert got[0][:6] == got[1][:6] and got[0][1] == d
    assert np.array_equal(got[0][6].reshape(n, n, order="F"), Lg)
    assert got[1][6].dtype == np.uint16 and np.array_equal(got[1][6], ref.convert_reference(got[0][6], 16))
    assert np.array_equal(got[0][7], got[1][7])


# ------------------------------------------------------------------ 3. device-resident narrow arrays
def _torch_labels(torch, a):
    """numpy label array -> CUDA tensor of the same bytes (uint16 tensors are made from their bytes)."""
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


@pytest.mark.parametrize("bits", [8, 16])
def test_jordan_reduce_into_a_device_resident_narrow_array(pkg, golden, setups, bits):
    import torch
    setup = setups["esc16j"]
    n, CL, X0L, U = setup
    Lg = golden["esc16j_P"]
    cw, cn = _pair(pkg, bits, seed=71)
    with cw, cn:
        tCL, tX0 = torch.from_numpy(CL).cuda(), torch.from_numpy(X0L).cuda()
        tU = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
        args = [C.c_void_p(t.data_ptr()) for t in (tCL, tX0, tU)]
        tPw = torch.zeros(n * n, dtype=torch.int32, device="cuda")
        tPn = torch.zeros(n * n * (bits // 8) + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rw = _jordan_reduce(cw, setup, C.c_void_p(tPw.data_ptr()), mem=DEVICE, args=args)
        # (the narrow array starts one element into its allocation: aligned to its element only)
        rn = _jordan_reduce(cn, setup, C.c_void_p(tPn.data_ptr() + bits // 8), mem=DEVICE, args=args)
        assert rw["status"] in (0, 2, 3)
        _same_reduction(rw, rn)  # (the images came from sdpsr_block_images after a sizes-only call)
        Pw = tPw.cpu().numpy().view(np.uint32)
        raw = tPn.cpu().numpy()
        Pn = raw[bits // 8:bits // 8 + n * n * (bits // 8)].copy().view(ref.DTYPES[bits])
        assert np.array_equal(Pw.reshape(n, n, order="F"), Lg) and np.array_equal(Pn, ref.convert_reference(Pw, bits))
        assert (raw[:bits // 8] == 0).all() and (raw[bits // 8 + n * n * (bits // 8):] == 0).all()


def test_desymmetrize_and_refine_on_device_arrays_at_width_16(pkg, golden):
    import torch
    Lg = golden["er7_P"]
    n, d = Lg.shape[0], int(Lg.max())
    flat = np.ascontiguousarray(Lg.ravel(order="F")).astype(np.uint16)
    other = np.ascontiguousarray(_parity_labels(n).ravel(order="F")).astype(np.uint16)
    with pkg.Context(seed=81, label_width=16) as ch, pkg.Context(seed=81, label_width=16) as cd:
        lib = ch._lib
        # desymmetrize
        hostP = flat.copy()
        dh, ih = C.c_int64(d), C.c_int32(0)
        ch.check(lib.sdpsr_desymmetrize(ch._h, n, _vp(hostP), C.byref(dh), C.byref(ih), HOST))
        tP = _torch_labels(torch, flat)
        torch.cuda.synchronize()
        dv, iv = C.c_int64(d), C.c_int32(0)
        cd.check(lib.sdpsr_desymmetrize(cd._h, n, C.c_void_p(tP.data_ptr()), C.byref(dv), C.byref(iv), DEVICE))
        assert (dh.value, ih.value) == (dv.value, iv.value)
        assert np.array_equal(tP.cpu().numpy().view(np.uint16), hostP)
        # refine
        d2 = int(other.max())
        hostP = flat.copy()
        dh = C.c_int64(d)
        ch.check(lib.sdpsr_refine(ch._h, n * n, _vp(hostP), C.byref(dh), _vp(other), d2, HOST))
        tP, tQ = _torch_labels(torch, flat), _torch_labels(torch, other)
        torch.cuda.synchronize()
        dv = C.c_int64(d)
        cd.check(lib.sdpsr_refine(cd._h, n * n, C.c_void_p(tP.data_ptr()), C.byref(dv), C.c_void_p(tQ.data_ptr()), d2, DEVICE))
        assert dh.value == dv.value and dh.value > d
        assert np.array_equal(tP.cpu().numpy().view(np.uint16), hostP)
        assert np.array_equal(tQ.cpu().numpy().view(np.uint16), other)  # p2 is an input


# ------------------------------------------------------------------ 4. the bytes that cross
@pytest.mark.parametrize("bits", [8, 16])
def test_transfer_bytes_count_the_narrow_arrays(pkg, golden, setups, bits):
    setup = setups["esc16j"]
    n = setup[0]
    Lg = golden["esc16j_P"]
    d = int(Lg.max())
    len_ = n * n
    deltas = {}
    for width in (32, bits):
        with pkg.Context(seed=91, label_width=width) as c:
            with pkg.Problem(setup=setup, ctx=c) as prob:
                h0, d0 = c.transfer_bytes()
                res = prob.reduce_batch(1, seeds=[3])[0]  # (two calls: sizes, then images)
                h1, d1 = c.transfer_bytes()
            assert res["status"] in (0, 2, 3)
            # blockDiagonalize from host labels
            P = pkg.Partition(d, Lg.astype(ref.DTYPES[width]))
            h2, d2 = c.transfer_bytes()
            nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
            lab = np.ascontiguousarray(P.matrix.ravel(order="F"))
            st = c._lib.sdpsr_block_diagonalize(c._h, n, _vp(lab), d, RTOL, C.byref(nb), C.byref(ssq), C.byref(ss), None, HOST)
            assert st in (0, 2, 3)
            h3, d3 = c.transfer_bytes()
            deltas[width] = (h1 - h0, d1 - d0, h3 - h2, d3 - d2, st, res["status"])
    w, nrw = deltas[32], deltas[bits]
    per_array = len_ * (4 - bits // 8)
    # Problem.reduce with host outputs: the sizes call and the images call each deliver P_out once -- two label arrays down,
    # none up; everything else (descriptors, class values, images) is the same at both widths (same seed, same draws)
    assert w[5] == nrw[5]
    assert w[0] - nrw[0] == 0
    assert w[1] - nrw[1] == 2 * per_array
    # blockDiagonalize: one label array up
    assert w[4] == nrw[4]
    assert w[2] - nrw[2] == per_array
    assert w[3] - nrw[3] == 0


# ------------------------------------------------------------------ 5. overflow: count set, labels untouched
@pytest.mark.parametrize("bits,classes", [(8, 255), (8, 256), (16, 65535), (16, 65536)])
def test_partition_from_u32_at_the_class_count_limit(pkg, bits, classes):
    len_ = max(classes, 4096) if bits == 8 else 65536
    keys = np.zeros(len_, dtype=np.uint32)
    keys[:classes] = np.random.default_rng(classes).permutation(classes).astype(np.uint32) + 1000  # all distinct, then zeros
    sentinel = ref.typemax(bits) - 1
    for mem in (HOST, DEVICE):
        with pkg.Context(seed=1, label_width=bits) as c:
            lib = c._lib
            out = np.full(len_, sentinel, dtype=ref.DTYPES[bits])
            nparts = C.c_int64(-1)
            if mem == HOST:
                st = lib.sdpsr_partition_from_u32(c._h, len_, _vp(keys), _vp(out), C.byref(nparts), HOST)
            else:
                import torch
                tk = torch.from_numpy(keys.view(np.int32)).cuda()
                to = _torch_labels(torch, out)
                torch.cuda.synchronize()
                st = lib.sdpsr_partition_from_u32(c._h, len_, C.c_void_p(tk.data_ptr()), C.c_void_p(to.data_ptr()), C.byref(nparts), DEVICE)
                out = to.cpu().numpy().view(ref.DTYPES[bits])
            assert nparts.value == classes
            if classes <= ref.typemax(bits):
                assert st == OK
                expect = np.zeros(len_, dtype=np.uint64)
                expect[:classes] = np.arange(1, classes + 1)  # labelled by first occurrence
                assert np.array_equal(out.astype(np.uint64), expect)
            else:
                assert st == LABEL_OVERFLOW
                assert (out == sentinel).all()
                # the ctx stays usable
                small = np.array([5, 5, 0, 9], dtype=np.uint32)
                o4 = np.zeros(4, dtype=ref.DTYPES[bits])
                assert lib.sdpsr_partition_from_u32(c._h, 4, _vp(small), _vp(o4), C.byref(nparts), HOST) == OK
                assert list(o4) == [1, 1, 0, 2] and nparts.value == 2


def test_refine_whose_meet_does_not_fit_8_bits(pkg):
    # 20 x 20 classes: rows and columns of a 20 x 20 grid (20 classes each); their meet has 400 > 255 classes
    i = np.arange(400)
    p1 = (i // 20 + 1).astype(np.uint8)
    p2 = (i % 20 + 1).astype(np.uint8)
    for mem in (HOST, DEVICE):
        with pkg.Context(seed=1, label_width=8) as c:
            lib = c._lib
            d1 = C.c_int64(20)
            if mem == HOST:
                a = p1.copy()
                st = lib.sdpsr_refine(c._h, 400, _vp(a), C.byref(d1), _vp(p2), 20, HOST)
            else:
                import torch
                ta, tb = torch.from_numpy(p1.copy()).cuda(), torch.from_numpy(p2.copy()).cuda()
                torch.cuda.synchronize()
                st = lib.sdpsr_refine(c._h, 400, C.c_void_p(ta.data_ptr()), C.byref(d1), C.c_void_p(tb.data_ptr()), 20, DEVICE)
                a = ta.cpu().numpy()
            assert st == LABEL_OVERFLOW and d1.value == 400
            assert np.array_equal(a, p1)
    with pkg.Context(seed=1, label_width=16) as c:
        a = p1.astype(np.uint16)
        d1 = C.c_int64(20)
        assert c._lib.sdpsr_refine(c._h, 400, _vp(a), C.byref(d1), _vp(p2.astype(np.uint16)), 20, HOST) == OK
        assert d1.value == 400 and np.array_equal(a, np.arange(1, 401).astype(np.uint16))


GNP_N, GNP_DIM = 23, 276  # the smallest n for which the oracle's admissible_subspace of theta'(gnp_adjacency(n)) has dim > 255
# (oracle on the CPU: n = 21, 22, 23, 24 -> dim 231, 253, 276, 300 = n (n + 1) / 2, a graph without symmetry)


@pytest.fixture(scope="module")
def gnp(pkg, problems, oracle):
    Cv, A, b = problems.theta_prime_problem(problems.gnp_adjacency(GNP_N))
    Po = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0))
    assert oracle.dim(Po) == GNP_DIM > 255
    return pkg.admissible_setup(Cv, A, b), np.asarray(Po.matrix).astype(np.uint32)


def test_admissible_subspace_and_jordan_reduce_overflow_at_width_8(pkg, gnp):
    setup, Lo = gnp
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    r = U.shape[1]
    sentinel = 0xEE
    with pkg.Context(seed=2, label_width=8) as c:
        lib = c._lib
        P = np.full(n * n, sentinel, dtype=np.uint8)
        dd, it = C.c_int64(0), C.c_int32(0)
        if setup.hint:
            lib.sdpsr_hint_symmetric_basis(c._h, setup.hint)
        st = lib.sdpsr_admissible_subspace(c._h, n, _vp(CL), _vp(X0L), _vp(Uf), r, RTOL, _vp(P), C.byref(dd), C.byref(it), None, HOST)
        assert st == LABEL_OVERFLOW and dd.value == GNP_DIM and (P == sentinel).all()
        with pytest.raises(pkg.LabelOverflow):
            pkg.admissible_subspace(None, None, None, ctx=c, setup=setup)
        res = _jordan_reduce(c, setup, P)
        assert res["status"] == LABEL_OVERFLOW and res["dim"] == GNP_DIM and (P == sentinel).all()
        assert res["nblocks"] == 0
        # a batch with R = 2 reports it in both status words
        R = 2
        Ps = [np.full(n * n, sentinel, dtype=np.uint8) for _ in range(R)]
        pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
        d2, st2 = (C.c_int64 * R)(), (C.c_int32 * R)()
        if setup.hint:
            lib.sdpsr_hint_symmetric_basis(c._h, setup.hint)
        rc = lib.sdpsr_jordan_reduce_batch(c._h, R, None, n, _vp(CL), _vp(X0L), _vp(Uf), r, RTOL, RTOL, C.cast(pP, C.c_void_p), d2, None, None, None, None,
                                           None, None, st2, HOST)
        assert rc == LABEL_OVERFLOW and list(st2) == [LABEL_OVERFLOW] * R and list(d2) == [GNP_DIM] * R
        assert all((a == sentinel).all() for a in Ps)
        with pkg.Problem(setup=setup, ctx=c) as prob:
            out = prob.reduce_batch(2, seeds=[1, 2])
            assert [x["status"] for x in out] == [LABEL_OVERFLOW] * 2
    with pkg.Context(seed=2, label_width=16) as c:
        P16 = pkg.admissible_subspace(None, None, None, ctx=c, setup=setup)
        assert P16.nparts == GNP_DIM and P16.matrix.dtype == np.uint16 and np.array_equal(P16.matrix, Lo)
        P = np.zeros(n * n, dtype=np.uint16)
        res = _jordan_reduce(c, setup, P, images=False)
        assert res["status"] in (0, 2, 3) and res["dim"] == GNP_DIM and np.array_equal(P.reshape(n, n, order="F"), Lo)


# ------------------------------------------------------------------ 6. the setter
def test_setter_validates_and_switching_equals_fresh_contexts(pkg, golden, setups):
    setup = setups["er7"]
    Lg = golden["er7_P"]
    with pkg.Context(seed=5) as c:
        lib = c._lib
        assert lib.sdpsr_label_width(c._h) == 32 and c.label_width == 32 and c.label_dtype == np.uint32
        for bad in (12, 0, 64, -8):
            assert lib.sdpsr_set_label_width(c._h, bad) == BAD_ARGUMENT
            assert lib.sdpsr_label_width(c._h) == 32
        with pytest.raises(ValueError):
            c.label_width = 12
        got = []
        for width in (32, 16, 32):
            c.label_width = width
            assert lib.sdpsr_label_width(c._h) == width
            c.set_seed(5)
            P = pkg.admissible_subspace(None, None, None, ctx=c, setup=setup)
            got.append((P.matrix.dtype, P.nparts, P.iterations, P.dims, P.matrix.copy(), pkg.randomize(P, ctx=c)))
        for width, g in zip((32, 16, 32), got):
            with pkg.Context(seed=5, label_width=width) as f:
                P = pkg.admissible_subspace(None, None, None, ctx=f, setup=setup)
                fresh = (P.matrix.dtype, P.nparts, P.iterations, P.dims, P.matrix.copy(), pkg.randomize(P, ctx=f))
            assert g[:4] == fresh[:4] and g[0] == ref.DTYPES[width]
            assert np.array_equal(g[4], fresh[4]) and np.array_equal(g[4], Lg) and np.array_equal(g[5], fresh[5])
    with pytest.raises(ValueError):
        pkg.Context(seed=1, label_width=12)
