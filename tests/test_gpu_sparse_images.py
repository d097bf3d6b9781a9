"""sdpsr_block_images_sparse: dense block images compacted into solver triplets on the device, against the NumPy restatement
(tests/sparse_images_ref.py).  Nothing is computed -- negation is the only arithmetic -- so every comparison is EXACT:
integers equal, values and max_asym bit for bit.  Every buffer the library reads or writes sits between guard elements."""
import ctypes as C
import functools

import numpy as np
import pytest

from basis_image_helpers import gaussian_unit_columns
from sparse_images_ref import max_asym_ref, sparse_ref, virtual_sizes

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT = 0, 5
HOST, DEVICE = 0, 1
UPPER, FULL = 0, 1
GUARD = 6          # elements on either side of every buffer; even: the guarded window stays 16-byte aligned on the device
IDX_GUARD = -7     # sentinel of the integer outputs
CHUNK = 2048       # SI_CHUNK (csrc/sparse_images.h): flat elements per wave, per count, per scan entry
LDS_BLOCKS = 2048  # SI_LDS_BLOCKS: the block table is searched in LDS up to this many blocks, in global memory beyond
SCAN_ROUND = 4096  # counts per round of the one-workgroup scan; it loops, so there is no single-level limit -- the case
                   # "beyond" is the first shape whose scan takes a second round: more than SCAN_ROUND * CHUNK elements


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(sizes, count, cx, density, seed, tol=0.0, special=False, nan=False):
    """count * sum s_k^2 seeded elements, a share `density` of them non-zero; special: +-tol, their neighbours and +-0.0 at random places."""
    rng = np.random.default_rng(seed)
    n = count * sum(s * s for s in sizes)
    comps = []
    for _ in range(2 if cx else 1):
        v = rng.standard_normal(n) * (rng.random(n) < density)
        if special and n:
            vals = [tol, -tol, np.nextafter(tol, 1), -np.nextafter(tol, 1), 0.0, -0.0, tol / 2, 5e-324] + ([np.nan, -np.nan] if nan else [])
            where = rng.integers(0, n, size=min(n, 4 * len(vals)))
            v[where] = np.resize(vals, where.size)
        comps.append(v)
    return comps[0] + 1j * comps[1] if cx else comps[0]


def _run(ctx, sizes, flat, upper=True, tol=0.0, base=0, mem=HOST, odd=False, capacity=0, null_arrays=False, asym=True, over=None):
    """One call of the C entry.  over: arguments replaced after everything is set up (the refusals).  Returns the status and
    every buffer as the call left it (device buffers copied back), guards included."""
    cx = np.iscomplexobj(flat)
    sz = np.asarray(sizes, dtype=np.int32)
    S = int(sum(int(s) * int(s) for s in sizes))
    src = np.ascontiguousarray(flat).view(np.float64)
    count = flat.size // S
    shift = GUARD + (1 if odd else 0)
    bufs = {"in": np.full(shift + src.size + GUARD, np.nan), "classptr": np.full(2 * GUARD + count + 1, IDX_GUARD, dtype=np.int64),
            "val": np.full(2 * GUARD + capacity, np.nan)}
    for k in ("blk", "row", "col"):
        bufs[k] = np.full(2 * GUARD + capacity, IDX_GUARD, dtype=np.int32)
    bufs["in"][shift:shift + src.size] = src
    pristine = bufs["in"].copy()
    if mem == DEVICE:
        import torch
        held = {k: torch.from_numpy(v).cuda() for k, v in bufs.items()}
        torch.cuda.synchronize()
        addr = {k: t.data_ptr() for k, t in held.items()}
    else:
        held = bufs
        addr = {k: v.ctypes.data for k, v in bufs.items()}
    ptr = {k: C.c_void_p(addr[k] + (shift if k == "in" else GUARD) * bufs[k].itemsize) for k in bufs}
    if null_arrays:
        for k in ("blk", "row", "col", "val"):
            ptr[k] = None
    nnz, am = C.c_int64(-1), C.c_double(-1.0)
    args = dict(nblocks=len(sz), sizes=C.c_void_p(sz.ctypes.data), count=count, blks=ptr["in"], cx=int(cx), tri=UPPER if upper else FULL,
                tol=float(tol), base=base, capacity=capacity, classptr=ptr["classptr"], blk=ptr["blk"], row=ptr["row"], col=ptr["col"],
                val=ptr["val"], nnz=C.byref(nnz), asym=C.byref(am) if asym else None, mem=mem)
    args.update(over or {})
    st = ctx._lib.sdpsr_block_images_sparse(ctx._h, *args.values())
    if mem == DEVICE:
        import torch
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in held.items()}
    else:
        out = bufs
    assert np.array_equal(_bits(out["in"]), _bits(pristine)), "the input changed"
    return {"status": st, "nnz": nnz.value, "asym": am.value, "count": count, "capacity": capacity, **{k: out[k] for k in out if k != "in"}}


def _guards_intact(r, written):
    """classptr's guards, and everything of the entry arrays outside the first `written` entries."""
    cp = r["classptr"]
    ok = (cp[:GUARD] == IDX_GUARD).all() and (cp[GUARD + r["count"] + 1:] == IDX_GUARD).all()
    for k in ("blk", "row", "col"):
        ok = ok and (np.delete(r[k], np.s_[GUARD:GUARD + written]) == IDX_GUARD).all()
    return bool(ok and np.isnan(np.delete(r["val"], np.s_[GUARD:GUARD + written])).all())


def _check(ctx, sizes, flat, ref=None, amax=None, **kw):
    """The sizing call and the filling call against the restatement; returns the filling call's buffers."""
    ref = ref or sparse_ref(flat, sizes, upper=kw.get("upper", True), tol=kw.get("tol", 0.0), index_base=kw.get("base", 0))
    has_nan = bool(np.isnan(np.ascontiguousarray(flat).view(np.float64)).any())
    want_asym = None if has_nan else (max_asym_ref(flat, sizes) if amax is None else amax)
    n = ref["nnz"]
    a = _run(ctx, sizes, flat, capacity=0, null_arrays=True, **kw)
    assert a["status"] == OK and a["nnz"] == n, (a["status"], a["nnz"], n)
    assert np.array_equal(a["classptr"][GUARD:GUARD + a["count"] + 1], ref["classptr"]) and _guards_intact(a, 0)
    b = _run(ctx, sizes, flat, capacity=n + 3, **kw)
    assert b["status"] == OK and b["nnz"] == n
    assert np.array_equal(b["classptr"][GUARD:GUARD + b["count"] + 1], ref["classptr"]) and _guards_intact(b, n)
    for k in ("blk", "row", "col"):
        assert np.array_equal(b[k][GUARD:GUARD + n], ref[k]), k
    assert np.array_equal(_bits(b["val"][GUARD:GUARD + n]), _bits(ref["val"]))
    if want_asym is not None:
        assert _bits([a["asym"]])[0] == _bits([want_asym])[0] == _bits([b["asym"]])[0], (a["asym"], want_asym)
    return b


SMALL = [([1, 2, 3], 7), ([3], 5), ([2, 1], 1), ([1], 3)]  # S = 14; S = 9, odd; one class; fewer elements than lanes


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("sizes,count", SMALL)
def test_small_shapes_every_option(gpu_ctx, sizes, count, cx):
    for tol in (0.0, 1e-8):
        for nan in (False, True):
            flat = _data(sizes, count, cx, 0.6, 17 + count, tol=tol, special=True, nan=nan)
            for upper in (True, False):
                for base in (0, 1):
                    _check(gpu_ctx, sizes, flat, upper=upper, tol=tol, base=base, mem=HOST)
                    for odd in (False, True):  # a window that starts at an odd element of a larger device buffer
                        _check(gpu_ctx, sizes, flat, upper=upper, tol=tol, base=base, mem=DEVICE, odd=odd)


@pytest.mark.parametrize("mem", [HOST, DEVICE])
def test_many_classes_in_one_chunk(gpu_ctx, mem):
    flat = _data([1], 5000, False, 0.5, 3)  # 5000 classes of one element: ~2048 class boundaries per chunk
    for odd in ((False, True) if mem == DEVICE else (False,)):
        _check(gpu_ctx, [1], flat, mem=mem, odd=odd, base=1)
    _check(gpu_ctx, [1], _data([1], 5000, True, 0.5, 4), mem=mem, upper=False)


def test_all_zero_all_kept_and_empty_classes(gpu_ctx):
    for sizes, count in (([1, 2, 3], 9), ([37, 63, 1], 3)):
        S = sum(s * s for s in sizes)
        for cx in (False, True):
            zero = np.zeros(count * S, dtype=np.complex128 if cx else np.float64)
            zero[1::2] = -0.0
            r = _check(gpu_ctx, sizes, zero, mem=DEVICE, upper=False)
            assert r["nnz"] == 0
            full = _data(sizes, count, cx, 1.0, 5)
            r = _check(gpu_ctx, sizes, full, mem=DEVICE, upper=False)
            assert r["nnz"] == count * sum(v * v for v in virtual_sizes(sizes, cx))
            holes = full.copy().reshape(count, S)
            holes[[0, 1, 4, 5, count - 1] if count == 9 else [0, 2]] = 0  # leading, consecutive and trailing empty classes
            _check(gpu_ctx, sizes, holes.reshape(-1), mem=DEVICE, odd=not cx)
            _check(gpu_ctx, sizes, holes.reshape(-1), mem=HOST, upper=False, base=1)
    # runs of empty classes longer than a chunk, leading and trailing
    v = _data([1], 5000, False, 0.5, 8)
    v[:3000] = 0
    v[4500:] = 0
    _check(gpu_ctx, [1], v, mem=DEVICE)


@functools.lru_cache(maxsize=None)
def _big(count, upper):
    sizes = [37, 63, 1]  # S = 5339: odd, no multiple of anything the kernels use
    flat = _data(sizes, count, False, 0.3, 21, tol=1e-8, special=True)
    flat.setflags(write=False)
    return sizes, flat, sparse_ref(flat, sizes, upper=upper, tol=1e-8, index_base=1), max_asym_ref(flat, sizes)


def test_three_blocks_three_classes(gpu_ctx):
    sizes = [37, 63, 1]
    for cx in (False, True):
        flat = _data(sizes, 3, cx, 0.3, 22, tol=1e-8, special=True)
        for upper in (True, False):
            _check(gpu_ctx, sizes, flat, upper=upper, tol=1e-8, mem=DEVICE, odd=True)
            _check(gpu_ctx, sizes, flat, upper=upper, tol=1e-8, mem=HOST, base=1)


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "full"])
def test_thousand_classes(gpu_ctx, upper):
    sizes, flat, ref, amax = _big(1000, upper)  # 5.3 M elements, 2607 chunks
    _check(gpu_ctx, sizes, flat, ref=ref, amax=amax, upper=upper, tol=1e-8, base=1, mem=DEVICE, odd=upper)


def test_scan_takes_a_second_round(gpu_ctx):
    count = 1600
    sizes, flat, ref, amax = _big(count, True)
    assert count * 5339 > SCAN_ROUND * CHUNK  # 4171 counts: more than one round of the scan
    _check(gpu_ctx, sizes, flat, ref=ref, amax=amax, upper=True, tol=1e-8, base=1, mem=DEVICE)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_more_blocks_than_the_lds_table_holds(gpu_ctx, cx):
    for nb in (LDS_BLOCKS, LDS_BLOCKS + 1):  # the last table in LDS, the first one in global memory
        sizes = [1] * (nb - 1) + [2]
        flat = _data(sizes, 3, cx, 0.5, 31)
        _check(gpu_ctx, sizes, flat, mem=DEVICE, base=1)
        _check(gpu_ctx, sizes, flat, mem=DEVICE, upper=False, odd=True)


def test_capacity_rule(gpu_ctx):
    sizes = [1, 2, 3]
    flat = _data(sizes, 40, False, 0.5, 41)
    ref = sparse_ref(flat, sizes)
    n = ref["nnz"]
    for mem in (HOST, DEVICE):
        r = _run(gpu_ctx, sizes, flat, capacity=n - 1, mem=mem)  # one entry short: nothing of the entries is written
        assert r["status"] == OK and r["nnz"] == n and _guards_intact(r, 0)
        assert np.array_equal(r["classptr"][GUARD:GUARD + 41], ref["classptr"])
        r = _run(gpu_ctx, sizes, flat, capacity=n, mem=mem)  # exactly enough
        assert r["status"] == OK and _guards_intact(r, n) and np.array_equal(r["row"][GUARD:GUARD + n], ref["row"])
    empty = _run(gpu_ctx, sizes, flat[:0], capacity=0, null_arrays=True, mem=HOST, over=dict(blks=None))
    assert empty["status"] == OK and empty["nnz"] == 0 and empty["asym"] == 0.0 and empty["classptr"][GUARD] == 0 and _guards_intact(empty, 0)
    empty = _run(gpu_ctx, sizes, flat[:0], capacity=0, null_arrays=True, mem=DEVICE)
    assert empty["status"] == OK and empty["nnz"] == 0 and empty["classptr"][GUARD] == 0 and _guards_intact(empty, 0)


def test_two_contexts_give_equal_bytes(pkg, gpu_ctx):
    sizes = [5, 1, 4]
    flat = _data(sizes, 300, True, 0.4, 51, tol=1e-8, special=True)
    n = sparse_ref(flat, sizes, tol=1e-8)["nnz"]
    with pkg.Context(seed=99) as other:
        runs = [_run(c, sizes, flat, tol=1e-8, capacity=n, mem=DEVICE) for c in (gpu_ctx, other, gpu_ctx)]
    for r in runs[1:]:
        assert r["status"] == OK and r["nnz"] == n == runs[0]["nnz"]
        for k in ("classptr", "blk", "row", "col", "val"):
            assert r[k].tobytes() == runs[0][k].tobytes(), k
        assert _bits([r["asym"]])[0] == _bits([runs[0]["asym"]])[0]


def test_refusals_leave_everything_alone(gpu_ctx):
    sizes = [2, 3]
    flat = _data(sizes, 4, False, 0.7, 61)
    n = sparse_ref(flat, sizes)["nnz"]
    bad_sizes = np.asarray([2, 0], dtype=np.int32)
    huge = np.asarray([46341, 46341], dtype=np.int32)
    wide = np.asarray([2 ** 31 - 1], dtype=np.int32)
    cases = [dict(sizes=None), dict(classptr=None), dict(nnz=None), dict(blks=None), dict(blk=None), dict(row=None), dict(col=None),
             dict(val=None), dict(nblocks=0), dict(sizes=C.c_void_p(bad_sizes.ctypes.data)), dict(count=-1), dict(tol=-1e-300),
             dict(tol=float("nan")), dict(base=2), dict(base=-1), dict(tri=2), dict(tri=-1), dict(capacity=-1),
             dict(sizes=C.c_void_p(huge.ctypes.data), count=2 ** 62),      # class_count * sum s_k^2 overflows int64
             dict(sizes=C.c_void_p(wide.ctypes.data), nblocks=1, cx=1)]    # a virtual order of 2^32 - 2
    for mem in (HOST, DEVICE):
        for over in cases:
            r = _run(gpu_ctx, sizes, flat, capacity=n, mem=mem, over=over)
            assert r["status"] == BAD_ARGUMENT, over
            assert _guards_intact(r, 0) and (r["classptr"] == IDX_GUARD).all(), over
            assert gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h)
        _check(gpu_ctx, sizes, flat, mem=mem)  # the ctx is usable


def test_transfer_bytes(gpu_ctx):
    sizes = [1, 2, 3]
    for cx in (False, True):
        flat = _data(sizes, 50, cx, 0.5, 71)
        n = sparse_ref(flat, sizes)["nnz"]
        window = flat.size * (16 if cx else 8)
        for capacity, down in ((0, 0), (n - 1, 0), (n + 10, n * 20)):  # nnz entries come down, never `capacity` of them
            h0, d0 = gpu_ctx.transfer_bytes()
            r = _run(gpu_ctx, sizes, flat, capacity=capacity, null_arrays=capacity == 0, mem=HOST)
            h1, d1 = gpu_ctx.transfer_bytes()
            assert r["status"] == OK and (h1 - h0, d1 - d0) == (window, 16 + 51 * 8 + down)
        h0, d0 = gpu_ctx.transfer_bytes()
        r = _run(gpu_ctx, sizes, flat, capacity=n, mem=DEVICE)
        h1, d1 = gpu_ctx.transfer_bytes()
        assert r["status"] == OK and (h1 - h0, d1 - d0) == (0, 16)


# ------------------------------------------------------------------ the Python entries
def test_block_images_sparse_python(pkg, gpu_ctx):
    import torch
    sizes = [2, 3, 1]
    for cx in (False, True):
        flat = _data(sizes, 6, cx, 0.5, 81)
        ref = sparse_ref(flat, sizes, upper=True, index_base=1)
        S = sum(s * s for s in sizes)
        nested = [[flat[i * S + o:i * S + o + s * s].reshape(s, s, order="F") for s, o in zip(sizes, (0, 4, 13))] for i in range(6)]
        for arg in (flat, nested, torch.from_numpy(flat).cuda(), [[torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in r] for r in nested]):
            sp, am = pkg.block_images_sparse(arg, sizes, index_base=1, ctx=gpu_ctx, return_asym=True)
            on_dev = not isinstance(sp.val, np.ndarray)
            assert on_dev == (arg is not flat and arg is not nested)
            get = (lambda t: t.cpu().numpy()) if on_dev else (lambda t: t)
            assert sp.nnz == ref["nnz"] and sp.sizes == virtual_sizes(sizes, cx) and am == max_asym_ref(flat, sizes)
            for k in ("classptr", "blk", "row", "col"):
                assert np.array_equal(get(getattr(sp, k)), ref[k]), k
            assert np.array_equal(_bits(get(sp.val)), _bits(ref["val"]))
            assert np.array_equal(get(sp.cls), np.repeat(np.arange(6), np.diff(ref["classptr"])) + 1)
            dense = sp.to_dense()
            full = pkg.block_images_sparse(arg, sizes, upper=False, ctx=gpu_ctx).to_dense()
            for i in range(6):
                for k in range(3):
                    assert np.array_equal(dense[i][k], np.triu(full[i][k]))
    empty = pkg.block_images_sparse(np.zeros(0), sizes, ctx=gpu_ctx)
    assert empty.nnz == 0 and list(empty.classptr) == [0] and empty.cls.size == 0


@functools.lru_cache(maxsize=None)
def _labels(name):
    from __graft_entry__ import load_package
    pr = load_package().problems
    if name == "COMM":  # commutative, n = 80, d = 18
        L, d = pr.kron_with_complete(pr.symmetric_circulant_labels(16), 5)
    else:
        L, d, _ = pr.known_blocks_instance(name)
    return np.asarray(L, dtype=np.int64), int(d)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("route", ["outer", "chunk"])
@pytest.mark.parametrize("name", ["COMM", "K17"])
def test_basis_image_sparse_equals_the_compacted_dense_call(pkg, name, route, cx):
    """On the outer and chunk routes a window of basis_image equals the slice of the full call bit for bit, so the windows'
    triplets put together are the triplets of the full-range dense images."""
    import torch
    L, d = _labels(name)
    n = L.shape[0]
    sizes = [3, 1, 2]
    Q = gaussian_unit_columns(n, sum(sizes), 7)
    if cx:
        Q = (Q + 1j * gaussian_unit_columns(n, sum(sizes), 8)) / np.sqrt(2.0)
    classes = None if name == "COMM" else (5, 7)
    first, count = (1, d) if classes is None else classes
    with pkg.Context(seed=3, basis_image_kernel=route) as ctx:
        P = pkg.Partition(d, L.astype(np.uint32))
        dense = pkg.basis_image((Q, sizes), P, ctx=ctx)[first - 1:first - 1 + count]
        flat = np.concatenate([b.ravel(order="F") for row in dense for b in row])
        Pt = pkg.Partition(d, torch.from_numpy(L.astype(np.int32)).cuda())
        for upper, tol in ((True, 0.0), (False, 1e-2)):
            ref = sparse_ref(flat, sizes, upper=upper, tol=tol)
            assert 0 < ref["nnz"]
            for parts in (1, 3, count + 2):  # more parts than classes: empty windows
                for part in (P, Pt):
                    sp = pkg.basis_image_sparse((Q, sizes), part, parts=parts, classes=classes, upper=upper, tol=tol, ctx=ctx)
                    on_dev = part is Pt
                    assert on_dev == (not isinstance(sp.val, np.ndarray))
                    get = (lambda t: t.cpu().numpy()) if on_dev else (lambda t: t)
                    assert sp.nnz == ref["nnz"] and sp.sizes == virtual_sizes(sizes, cx)
                    for k in ("classptr", "blk", "row", "col"):
                        assert np.array_equal(get(getattr(sp, k)), ref[k]), (k, parts)
                    assert np.array_equal(_bits(get(sp.val)), _bits(ref["val"])), parts
