"""One refinement over every computed signature source (csrc/sig_sources.h), driven on made-up inputs through libsdpsr_prof.so
(sdpsr_profile_refine_source): the insert kernel of each of the 24 computed functor instances, its materialise kernel, the stand-alone
kernels of run-time shape, the mid kernel of the two sources that have one, and the driver of primitives.cpp around them (the
one-workgroup ranking and its repeat, the overflow repeat on labels refined in place, "ref_first", the fused symmetry verdict).

The reference (tests/refine_source_ref.py) gives every entry an exact key tuple and numbers the classes of equal tuples by first
occurrence; the inputs are exact (dyadic U and coef), so every case asserts, bit for bit: the labels -- with padding, guard and a
label array the refinement only reads untouched --, the class count, and "ref_first" wherever the ctx says it describes the result
(everywhere but behind the radix sort, which writes none).

Shapes: n = 5 (one 256-row step of the walk wraps dozens of columns), 57, 257 (packed: 33 153 entries = 16 chunks of 2048 and a
ragged tail whose last columns hold one or two entries); the mid kernel needs 2^20 entries: n = 1450 packed, 1030 unpacked."""
import ctypes as C

import numpy as np
import pytest

import refine_source_ref as R

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 5
GUARD = 40
GUARD_WORD, FILL = 0xA5A5A5A5, 0xDEADBEEF
FLAG_REFINE_NO_FUSE = 1 << 3


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def ctxs(pkg, gpu_ctx):
    """name -> ctx, made on first use: the session's default ctx and the ones that force a path."""
    spec = {"no_fuse": dict(flags=FLAG_REFINE_NO_FUSE), "trunc": dict(round_mode="trunc"),
            "trunc_no_fuse": dict(round_mode="trunc", flags=FLAG_REFINE_NO_FUSE), "bucket": dict(refine_path="bucket"),
            "sort": dict(refine_path="sort"), "no_mid": dict(refine_path="no_mid"), "mid_no_first": dict(refine_path="mid_no_first")}
    made = {"default": gpu_ctx}

    def get(name):
        if name not in made:
            made[name] = pkg.Context(device=0, seed=99, **spec[name])
        return made[name]
    yield get
    for name, ctx in made.items():
        if name != "default":
            ctx.close()


def _call(pkg, ctx, case, what=0, prev=34, sym=0, want_sig=False):
    """-> status, dict(new labels, nparts, first, report, sig); asserts that nothing but the new labels was written."""
    prof = pkg._lib.load_prof_library()
    kind, n, packed, lab_packed = case["kind"], case["n"], case["packed"], case["lab_packed"]
    nent = len(R.entries(n, packed)[0])
    apart = kind != "pair" and packed and not lab_packed
    L0 = np.ascontiguousarray(case["L"], dtype=np.uint32)
    Lio = np.concatenate([L0, np.full(GUARD, GUARD_WORD, dtype=np.uint32)])
    Lnew = np.full(nent + GUARD, FILL, dtype=np.uint32) if apart else None
    if apart:
        Lnew[nent:] = GUARD_WORD
    sig = np.zeros(nent, dtype=np.uint64) if want_sig else None
    first = np.full(R.FIRST_CAP, 0xFFFFFFFF, dtype=np.uint32)
    nparts, report = C.c_int64(-1), (C.c_int32 * 3)(-9, -9, -9)
    arr = {k: (np.ascontiguousarray(case[k]) if k in case else None) for k in ("a", "b", "U", "coef", "C")}
    if arr["C"] is not None:
        assert arr["C"].dtype == (np.float32 if kind == "chan_f32" else np.int32)
    st = prof.sdpsr_profile_refine_source(ctx._h, R.KINDS[kind], what, n, case["ld"], case["T"], case["r"], packed, lab_packed, C.c_uint64(case["key"]),
                                          case["atol"], _vp(arr["a"]), _vp(arr["b"]), _vp(arr["U"]), _vp(arr["coef"]), _vp(arr["C"]), _vp(Lio),
                                          _vp(Lnew), GUARD, prev, sym, _vp(sig), C.byref(nparts), _vp(first), report)
    if st != 0:
        assert np.array_equal(Lio[:len(L0)], L0) and (Lio[len(L0):] == GUARD_WORD).all()
        return st, None
    assert (Lio[len(L0):] == GUARD_WORD).all()
    if apart:
        assert np.array_equal(Lio[:len(L0)], L0) and (Lnew[nent:] == GUARD_WORD).all()  # the labels read stay; the guard behind the ones written
    new = (Lnew if apart else Lio)[:nent]
    return 0, dict(labels=new, nparts=int(nparts.value), first=first, report=[int(v) for v in report], sig=sig)


def _check(pkg, ctx, case, ref, what=0, prev=34, sym=0, want_sig=False, tag=None, has_first=True):
    st, out = _call(pkg, ctx, case, what=what, prev=prev, sym=sym, want_sig=want_sig)
    assert st == 0, (tag, st, ctx._lib.sdpsr_last_error(ctx._h).decode())
    lab, nparts, first = ref
    bad = np.flatnonzero(out["labels"] != lab)
    assert len(bad) == 0, (tag, len(bad), bad[:5], out["labels"][bad[:5]], lab[bad[:5]])
    assert out["nparts"] == nparts, tag
    assert out["report"][2] == (1 if has_first and nparts <= R.FIRST_CAP else 0), tag
    if out["report"][2]:
        assert np.array_equal(out["first"][:nparts], first), tag
        assert (out["first"][nparts:] == 0xFFFFFFFF).all(), tag
    return out


# ---- every instance once, fused and materialised ----
INSTANCES = ([("pair", 0, 0)] + [("proj", r, 0) for r in range(5)] + [(k, 0, T) for k in ("chan_i32", "chan_f32") for T in (1, 2, 4, 8)]
             + [("joint", r, T) for r in range(5) for T in (2, 4)])
LAYOUTS = {"pair": ((1, 1), (0, 0)), "proj": ((1, 1), (1, 0), (0, 0)), "chan_i32": ((1, 1), (1, 0), (0, 0)), "chan_f32": ((1, 1), (1, 0), (0, 0)),
           "joint": ((1, 1), (1, 0))}


assert len(INSTANCES) == len(set(INSTANCES)) == 24  # 1 + 5 + 8 + 10 computed sources; SrcArray is with_source's 25th functor


@pytest.mark.parametrize("n", [5, 57, 257])
@pytest.mark.parametrize("kind,r,T", INSTANCES, ids=[f"{k}-r{r}-T{T}" for k, r, T in INSTANCES])
def test_every_instance_fused_and_materialised(pkg, ctxs, kind, r, T, n):
    for packed, lab_packed in LAYOUTS[kind]:
        nent = n * (n + 1) // 2 if packed else n * n
        classes = 34 if nent >= 400 else 4
        case = R.make_case(kind, n, T=T, r=r, packed=packed, lab_packed=lab_packed, seed=1000 * n + 10 * r + T + packed + lab_packed, classes=classes)
        ref = R.refine_reference(case)
        assert (ref[1] > classes or (r == 0 and T == 0)) and ref[1] >= classes and (ref[0] == 0).any()  # the old classes do split, and a zero class is there
        for name in ("default", "no_fuse"):
            _check(pkg, ctxs(name), case, ref, tag=(kind, r, T, n, packed, lab_packed, name))


def test_pair_signed_zeros_and_last_bit_neighbours_are_classes_of_their_own(pkg, ctxs):
    case = R.make_case("pair", 57, packed=1, lab_packed=1, seed=3)
    ii, jj = R.entries(57, 1)
    a, b = case["a"][jj * 57 + ii], case["b"][jj * 57 + ii]
    ref = R.refine_reference(case)
    out = _check(pkg, ctxs("default"), case, ref)["labels"]
    sa, sb = np.signbit(a), np.signbit(b)
    za, zb = a == 0, b == 0
    assert np.array_equal(out == 0, za & zb & ~sa & ~sb)
    groups = [za & zb & sa & ~sb, za & zb & ~sa & sb, za & zb & sa & sb, (a == 0.7431) & zb & ~sb, (a == np.nextafter(0.7431, 2.0)) & zb & ~sb]
    labs = []
    for g in groups:
        assert g.any() and len(set(out[g])) == 1
        labs.append(int(out[g][0]))
    assert len(set(labs)) == 5 and 0 not in labs


# ---- planted edge values of the rounded projection, both rounding rules ----
@pytest.mark.parametrize("mode", ["nearest", "trunc"])
@pytest.mark.parametrize("kind,packed,lab_packed", [("proj", 1, 1), ("proj", 0, 0), ("joint", 1, 1)])
def test_planted_edge_values(pkg, ctxs, kind, packed, lab_packed, mode):
    case = R.make_planted_case(kind, 57, mode, packed=packed, lab_packed=lab_packed, seed=21)
    ref = R.refine_reference(case)
    for name in (("default", "no_fuse") if mode == "nearest" else ("trunc", "trunc_no_fuse")):
        out = _check(pkg, ctxs(name), case, ref, tag=(kind, mode, name))["labels"]
        y, l = R.projected(case), R.old_labels(case)
        below = y == np.nextafter(R.ATOL, 0.0)
        assert (out[below & (l == 0)] == 0).all() and (out[below & (l == R.TINY_LABEL)] != 0).all()
        assert (out[(y == R.ATOL) & (l == 0)] != 0).all()
        same = int(out[(y == 0.25) & (l == 0)][0]) == int(out[(y == 0.25 - 2.0 ** -32) & (l == 0)][0])
        assert same == (mode == "nearest")


# ---- one-entry needles ----
def _places(case):
    """name -> entry: first column, last row, last diagonal entry, an entry of label 0."""
    n, packed = case["n"], case["packed"]
    ii, jj = R.entries(n, packed)
    l = R.old_labels(case) if case["kind"] != "pair" else R.refine_reference(case)[0]
    return {"first_column": int(np.flatnonzero((jj == 0) & (ii == n // 2))[0]), "last_row": int(np.flatnonzero((ii == n - 1) & (jj == n // 3))[0]),
            "last_diagonal": len(ii) - 1, "label_zero": int(np.flatnonzero(l == 0)[-1])}


def _needle(case, e, comp):
    """A copy of the case that differs at entry e in one component: ("c", t), ("u",), ("a",) or ("b",)."""
    n, ld = case["n"], case["ld"]
    ii, jj = R.entries(n, case["packed"])
    i, j = int(ii[e]), int(jj[e])
    new = dict(case)
    if comp[0] == "c":
        Cn = case["C"].copy()
        at = comp[1] * ld * ld + j * ld + i
        Cn[at] = Cn[at] + 1 if Cn[at] < 1000 else Cn[at] - 1
        new["C"] = Cn
    elif comp[0] == "u":
        Un = case["U"].copy()
        at = (case["r"] - 1) * n * n + j * n + i
        scale = R.round_scale(case["atol"], case["round_mode"])
        for step in (512, 256, 384, 128, 640):
            Un[at] = case["U"][at] + (step if case["U"][at] < 0 else -step) / 1024.0
            new["U"] = Un
            if R._margins_ok(R.projected(new)[e], case["atol"], scale):
                break
        else:
            raise AssertionError("no needle value keeps the margins")
        R.check_exact_projection(Un, case["coef"])
    else:
        Mn = case[comp[0]].copy()
        at = j * n + i if case["packed"] else e
        Mn.view(np.uint64)[at] ^= np.uint64(2)  # (one bit; no value of the case's pools)
        new[comp[0]] = Mn
    return new


NEEDLE_SOURCES = ([("pair", 0, 0)] + [("proj", r, 0) for r in (1, 4)] + [(k, 0, T) for k in ("chan_i32", "chan_f32") for T in (1, 2, 4, 8)]
                  + [("joint", r, T) for r in (1, 4) for T in (2, 4)])


@pytest.mark.parametrize("kind,r,T", NEEDLE_SOURCES, ids=[f"{k}-r{r}-T{T}" for k, r, T in NEEDLE_SOURCES])
def test_one_entry_needles(pkg, ctxs, kind, r, T):
    n = 57
    base = R.make_case(kind, n, T=T, r=r, packed=1, lab_packed=1, seed=77 + 10 * r + T, classes=34, subs=1)
    ref0 = R.refine_reference(base)
    if kind != "pair":
        assert np.array_equal(ref0[0], base["L"])  # the new partition is the old one
    comps = [("a",), ("b",)] if kind == "pair" else ([("u",)] if r else []) + [("c", t) for t in range(T)]
    for name in ("default", "no_fuse"):
        _check(pkg, ctxs(name), base, ref0, tag=(kind, "base", name))
        for place, e in _places(base).items():
            for comp in comps:
                case = _needle(base, e, comp)
                ref = R.refine_reference(case)
                # exactly one more class, at that entry alone; everybody else keeps the partition
                assert ref[1] == ref0[1] + 1 and int((ref[0] == ref[0][e]).sum()) == 1 and ref[0][e] != 0, (place, comp)
                rest = np.arange(len(ref[0])) != e
                assert np.array_equal(R.canonical([ref[0][rest].astype(np.uint64)], ref[0][rest] == 0)[0],
                                      R.canonical([ref0[0][rest].astype(np.uint64)], ref0[0][rest] == 0)[0])
                _check(pkg, ctxs(name), case, ref, tag=(kind, r, T, place, comp, name))


# ---- the same bits from the functor and from the stand-alone kernel of run-time shape ----
@pytest.mark.parametrize("kind,r,T,layouts", [("chan_i32", 0, T, LAYOUTS["chan_i32"]) for T in (1, 2, 4, 8)]
                         + [("chan_f32", 0, T, LAYOUTS["chan_f32"]) for T in (1, 2, 4, 8)] + [("proj", r, 0, ((0, 0),)) for r in range(5)],
                         ids=[f"chan_i32-T{T}" for T in (1, 2, 4, 8)] + [f"chan_f32-T{T}" for T in (1, 2, 4, 8)] + [f"proj-r{r}" for r in range(5)])
def test_functor_and_standalone_kernel_give_the_same_bits(pkg, ctxs, kind, r, T, layouts):
    for packed, lab_packed in layouts:
        case = R.make_case(kind, 57, T=T, r=r, packed=packed, lab_packed=lab_packed, seed=5 + T + r)
        ref = R.refine_reference(case)
        o0 = _check(pkg, ctxs("default"), case, ref, what=0, want_sig=True)
        o1 = _check(pkg, ctxs("default"), case, ref, what=1, want_sig=True)
        assert np.array_equal(o0["sig"], o1["sig"]), (kind, r, T, packed, lab_packed)
        # classes of equal signature words are the reference's classes (no collision at this size), 0 exactly on the zero class
        assert np.array_equal(o0["sig"] == 0, ref[0] == 0) and len(np.unique(o0["sig"][ref[0] != 0])) == ref[1]


@pytest.mark.parametrize("kind,r,T,packed", [("chan_i32", 0, 3, 1), ("chan_f32", 0, 3, 0), ("chan_i32", 0, 5, 0), ("proj", 5, 0, 0)])
def test_shapes_without_a_functor_refine_through_the_standalone_kernel(pkg, ctxs, kind, r, T, packed):
    case = R.make_case(kind, 57, T=T, r=r, packed=packed, lab_packed=packed, seed=9)
    ref = R.refine_reference(case)
    for name in ("default", "no_fuse"):
        _check(pkg, ctxs(name), case, ref, tag=name)


def test_sources_nobody_can_write_out_are_refused(pkg, ctxs):
    ctx = ctxs("default")
    assert _call(pkg, ctx, R.make_case("proj", 57, r=5, packed=1, lab_packed=1, seed=1))[0] == BAD_ARGUMENT
    joint = R.make_case("joint", 57, r=1, T=2, packed=1, lab_packed=1, seed=1)
    flat = dict(joint, packed=0, lab_packed=0, L=np.resize(joint["L"], 57 * 57))
    assert _call(pkg, ctx, flat)[0] == BAD_ARGUMENT
    for what1 in (R.make_case("pair", 57, seed=1), joint, R.make_case("proj", 57, r=2, packed=1, lab_packed=1, seed=1)):
        assert _call(pkg, ctx, what1, what=1)[0] == BAD_ARGUMENT  # no stand-alone kernel for these
    assert _call(pkg, ctx, dict(joint, ld=joint["ld"] + 64))[0] == BAD_ARGUMENT


# ---- the driver's repeats on labels refined in place ----
@pytest.fixture(scope="module")
def count_cases():
    made = {}

    def get(kind, n, ncl, **kw):
        k = (kind, n, ncl, tuple(sorted(kw.items())))
        if k not in made:
            case = R.make_count_case(kind, n, ncl, seed=ncl + n, **kw)
            made[k] = (case, R.refine_reference(case))
        return made[k]
    return get


@pytest.mark.parametrize("ncl", [1024, 1025, 3072, 3073, "half"])
@pytest.mark.parametrize("kind", ["joint", "chan_i32"])
def test_driver_repeats_on_an_aliased_source(pkg, ctxs, count_cases, kind, ncl):
    case, ref = count_cases(kind, 257, 1000, distinct_in=16) if ncl == "half" else count_cases(kind, 257, ncl)
    true = ref[1]
    assert true == ncl if ncl != "half" else 33153 // 3 < true < 33153
    ctx = ctxs("default")
    guessed = _check(pkg, ctx, case, ref, prev=34, tag=(kind, ncl, "guessed"))["report"][0]
    # 34 classes predicted: a table of 2^12 slots and the one-workgroup ranking alone.  That ranking takes 1024 classes: one more and the
    # pass is repeated with the general ranking (the misprediction repeat, 1025 .. 3070 classes).  The table raises its overflow flag
    # with the 3071st distinct signature (more than 2047 + 1023 slots taken): from 3071 classes on -- 3072 and 3073 alike -- it is the
    # overflow repeat with the full-size table (len < 2^16).  Either repeat reads the old labels from the array again; the pass count
    # is 2 for both, which of the two ran follows from the thresholds above, not from the count.
    assert guessed == (1 if true <= 1024 else 2)
    assert _check(pkg, ctx, case, ref, prev=true, tag=(kind, ncl, "predicted"))["report"][0] == 1
    if ncl == 3073:
        _check(pkg, ctxs("bucket"), case, ref, prev=34, tag=(kind, "bucket"))
        assert _check(pkg, ctxs("sort"), case, ref, prev=34, tag=(kind, "sort"), has_first=False)["report"][0] == 1


@pytest.mark.parametrize("kind", ["joint", "chan_i32"])
def test_one_chunk_with_more_signatures_than_half_the_lds_table(pkg, ctxs, count_cases, kind):
    case, ref = count_cases(kind, 257, 700, dense_chunk=600)
    assert len(np.unique(ref[0][:2048])) >= 600
    for prev in (34, 700):
        assert _check(pkg, ctxs("default"), case, ref, prev=prev, tag=(kind, prev))["report"][0] == 1


# ---- the mid kernel with computed sources ----
@pytest.mark.parametrize("ncl", [40, 3000, 7000])
@pytest.mark.parametrize("kind,n,packed", [("pair", 1450, 1), ("chan_i32", 1450, 1), ("chan_i32", 1030, 0)])
def test_mid_kernel_with_computed_sources(pkg, ctxs, kind, n, packed, ncl):
    case = R.make_count_case(kind, n, ncl, seed=ncl + n, packed=packed, lab_packed=packed, last_alone=True)
    ref = R.refine_reference(case)
    assert ref[1] == ncl and int(ref[2][-1]) == len(ref[0]) - 1 >= (1 << 20) - 1
    # Which of the six runs go through refine_insert_mid_kernel over the COMPUTED source (primitives.cpp: mid = the source has one,
    # log2cap <= 16, len >= 2^20, refine_path != no_mid; nothing the entry reports tells, this is read off the driver):
    #   "default" / "mid_no_first", prev = 34: the first pass does, on a table of 2^12 slots.  At 40 classes the labels come from it; at
    #     3000 and 7000 it overflows, the source is written out and sampled, and the labels come from a pass over that ARRAY (mid again).
    #   "default" / "mid_no_first", prev = ncl: log2cap = 12, 15, 16 -- the labels come from the computed-source mid kernel in one pass.
    #   "no_mid": never; the plain insert kernel of the source, same labels.
    for name in ("default", "no_mid", "mid_no_first"):
        for prev in (34, ncl):  # guessed, then predicted
            _check(pkg, ctxs(name), case, ref, prev=prev, tag=(kind, n, ncl, name, prev))


# ---- the symmetry verdict fused into the label pass ----
def _mirror(n, ld, tri):
    """The full symmetric source of a packed chan case."""
    ii, jj = R.entries(n, 1)
    L = np.zeros(n * n, dtype=np.uint32)
    L[jj * n + ii] = tri["L"]
    L[ii * n + jj] = tri["L"]
    Cn = tri["C"].copy()
    for t in range(tri["T"]):
        Cn[t * ld * ld + ii * ld + jj] = Cn[t * ld * ld + jj * ld + ii]
    return dict(tri, packed=0, lab_packed=0, L=L, C=Cn)


@pytest.mark.parametrize("n", [64, 65, 132])
def test_fused_symmetry_verdict(pkg, ctxs, n):
    tri = R.make_case("chan_i32", n, T=2, packed=1, lab_packed=1, seed=n)
    full = _mirror(n, tri["ld"], tri)
    ref = R.refine_reference(full)
    assert np.array_equal(ref[0].reshape(n, n), ref[0].reshape(n, n).T)
    broken = dict(full, C=full["C"].copy())
    broken["C"][(n - 2) * tri["ld"] + n - 1] += 1  # row n - 1 of column n - 2: the last tile, off the diagonal
    refb = R.refine_reference(broken)
    assert refb[1] == ref[1] + 1 and not np.array_equal(refb[0].reshape(n, n), refb[0].reshape(n, n).T)
    for name in ("default", "no_fuse"):
        assert _check(pkg, ctxs(name), full, ref, sym=1, tag=(n, name))["report"][1] == 1
        assert _check(pkg, ctxs(name), broken, refb, sym=1, tag=(n, name, "broken"))["report"][1] == 0
    assert _check(pkg, ctxs("default"), full, ref, sym=0)["report"][1] == -1
