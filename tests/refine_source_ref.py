"""Exact NumPy reference of ONE refinement over a computed signature source (csrc/sig_sources.h: SrcPair, SrcProj<r>,
SrcChan<CT, T>, SrcJoint<r, T>), and the generators of the inputs that tests/test_gpu_refine_sources.py hands to
sdpsr_profile_refine_source.  Shared with tests/test_refine_source_ref_cpu.py.  Nothing here touches the library.

Every entry of the source -- in the source's own numbering: flat, or the packed lower triangle column by column -- gets an exact
key tuple:

    pair     (bits(a), bits(b))                    zero class: both words 0 (+0.0, not -0.0)
    proj     (l, code)                             zero class: l == 0 and code == 0
    chan     (l, c_0 .. c_{T-1})                   zero class: l == 0 and every channel 0
    joint    (l, code, c_0 .. c_{T-1})             zero class: all of it 0

with l the old label and code = sdpsr_round_key(x(l) - sum_k U_k coef_k).  Entries with equal tuples form a class; the classes are
numbered by first occurrence, the zero class is label 0 and is not counted.  The reference compares CLASSES: no hash value is
formed here (signature bits are only ever compared kernel against kernel).

No tolerance exists because the inputs are exact: U entries are integers / 2^10 and coef entries integers / 2^6, magnitudes below
1, so p = sum_k u_k coef_k is an integer / 2^16 of magnitude < 8 whichever way it is summed, with or without fma, and
y = x - p is ONE correctly rounded subtraction on both sides.  check_exact_projection asserts that contract."""
import numpy as np

from module_kernels_ref import GOLDEN, M64, class_uniform, fmix64

ATOL = 2.0 ** -26  # = sqrt(eps), the library's default tolerance (1.4901161193847656e-08): seven digits
KEY = 0x5DEECE66D1234567
KINDS = {"pair": 0, "proj": 1, "chan_i32": 2, "chan_f32": 3, "joint": 4}
INT32_MIN = -2 ** 31
FIRST_CAP = 65536  # REFINE_FIRST_CAP
SMALL_K = 1024     # classes the one-workgroup ranking takes


def round_scale(atol, mode="nearest"):
    """round_scale of ctx.cpp: 10^floor(-log10 atol), negative under truncation."""
    sc = 10.0 ** int(np.floor(-np.log10(atol)))
    return -sc if mode == "trunc" else sc


def round_key(a, atol, scale):
    """sdpsr_round_key on float64 arrays: 0 below atol, else (k, e) in a 52-bit and a 12-bit two's complement field."""
    a = np.asarray(a, dtype=np.float64)
    trunc = scale < 0
    sc = abs(float(scale))
    x, e = np.frexp(a)
    t = sc * x
    kd = np.trunc(t) if trunc else np.rint(t)
    fold = np.abs(kd) == sc  # the mantissa rounded up to 1.0: the same double as 0.5 * 2^(e + 1)
    kd = np.where(fold, kd * 0.5, kd)
    e = e.astype(np.int64) + fold
    code = (kd.astype(np.int64).view(np.uint64) & np.uint64((1 << 52) - 1)) | ((e.view(np.uint64) & np.uint64(0xFFF)) << np.uint64(52))
    return np.where(np.abs(a) < atol, np.uint64(0), code)


def scaled_mantissa(a, scale):
    return abs(float(scale)) * np.frexp(np.asarray(a, dtype=np.float64))[0]


def fmix64_inverse(z):
    """The inverse of sdpsr_fmix64 (a bijection of the 64-bit words), on Python ints."""
    def unshift(v, s):
        r, k = v, s
        while k < 64:
            r ^= v >> k
            k += s
        return r
    z = unshift(z, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & M64
    z = unshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M64
    return unshift(z, 30)


def key_with_uniform(label, m):
    """The key under which sdpsr_class_uniform(key, label) == m / 2^53."""
    return (fmix64_inverse((m << 11) & M64) - GOLDEN * label) & M64


# ---- numbering ----
_IJ = {}


def entries(n, packed):
    """(row, column) of every entry in the source's numbering."""
    k = (n, bool(packed))
    if k not in _IJ:
        cols = np.arange(n)
        if packed:
            _IJ[k] = (np.concatenate([np.arange(j, n) for j in range(n)]), np.repeat(cols, n - cols))
        else:
            _IJ[k] = (np.tile(cols, n), np.repeat(cols, n))
    return _IJ[k]


def col_off(n, j):
    return j * n - j * (j - 1) // 2


# ---- key tuples ----
def old_labels(case):
    n, ii, jj = case["n"], *entries(case["n"], case["packed"])
    L = case["L"]
    return (L[:len(ii)] if case["lab_packed"] or not case["packed"] else L[jj * n + ii]).astype(np.uint64)


def check_exact_projection(U, coef):
    Ui, ci = U * 1024.0, coef * 64.0
    assert np.array_equal(Ui, np.rint(Ui)) and np.array_equal(ci, np.rint(ci)) and np.abs(U).max(initial=0) < 1 and np.abs(coef).max(initial=0) < 1
    assert len(coef) <= 8


def projected(case):
    """y = x(l) - sum_k U_k coef_k at every entry (meaningful where the inputs are exact, see the module docstring)."""
    n, r = case["n"], case["r"]
    ii, jj = entries(n, case["packed"])
    ef = jj * n + ii
    p = np.zeros(len(ii))
    for k in range(r):
        p = p + case["U"][k * n * n + ef] * case["coef"][k]
    return class_uniform(case["key"], old_labels(case)) - p


def key_columns(case):
    """The columns of the key tuples (uint64 each) and the mask of the zero class."""
    kind, n = case["kind"], case["n"]
    ii, jj = entries(n, case["packed"])
    if kind == "pair":
        ef = jj * n + ii if case["packed"] else np.arange(n * n)
        ka, kb = case["a"].view(np.uint64)[ef], case["b"].view(np.uint64)[ef]
        return [ka, kb], (ka == 0) & (kb == 0)
    l = old_labels(case)
    cols, zero = [l], l == 0
    if kind in ("proj", "joint"):
        code = round_key(projected(case), case["atol"], round_scale(case["atol"], case["round_mode"]))
        cols.append(code)
        zero = zero & (code == 0)
    if kind != "proj":
        ld, C = case["ld"], case["C"]
        for t in range(case["T"]):
            c = C[t * ld * ld + jj * ld + ii]
            ci = c.astype(np.int64)
            assert np.array_equal(ci, c)  # f32 channels hold integers (< 2^24)
            cols.append(ci.view(np.uint64))
            zero = zero & (ci == 0)
    return cols, zero


def canonical(cols, zero):
    """labels (uint32), nparts, first_idx (uint32, class l at [l - 1]) of the classes of equal key tuples, by first occurrence."""
    g = np.zeros(len(cols[0]), dtype=np.int64)
    for c in cols:
        _, inv = np.unique(c, return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        _, g = np.unique(g * (int(inv.max()) + 1) + inv, return_inverse=True)
        g = g.reshape(-1).astype(np.int64)
    order = np.argsort(g, kind="stable")
    starts = np.flatnonzero(np.concatenate([[True], g[order][1:] != g[order][:-1]]))
    first = order[starts]  # first occurrence of group k at [k]
    is_zero = zero[first]
    assert np.array_equal(zero, is_zero[g])
    nz = np.flatnonzero(~is_zero)
    rank = np.argsort(first[nz], kind="stable")
    lab_of_group = np.zeros(len(first), dtype=np.uint32)
    lab_of_group[nz[rank]] = np.arange(1, len(nz) + 1, dtype=np.uint32)
    return lab_of_group[g], len(nz), first[nz][rank].astype(np.uint32)


def refine_reference(case):
    return canonical(*key_columns(case))


def scan_reference(cols, zero):
    """The same by a plain scan, for small cases."""
    seen, labels, first = {}, [], []
    for e in range(len(cols[0])):
        if zero[e]:
            labels.append(0)
            continue
        t = tuple(int(c[e]) for c in cols)
        if t not in seen:
            seen[t] = len(seen) + 1
            first.append(e)
        labels.append(seen[t])
    return np.array(labels, dtype=np.uint32), len(seen), np.array(first, dtype=np.uint32)


# ---- generators ----
def _canonical_old_labels(rng, nent, classes, zero_region=True):
    """Old labels 0 .. classes over nent entries, numbered by first occurrence, with a run of label 0 in the middle as well."""
    l = rng.integers(0 if zero_region else 1, classes + 1, size=nent)
    l[:classes] = rng.permutation(classes) + 1
    if zero_region:
        l[nent // 2:nent // 2 + max(1, nent // 16)] = 0
    lab, _, _ = canonical([l.astype(np.uint64)], l == 0)
    return lab.astype(np.int64)


def _margins_ok(y, atol, scale):
    """The contract of the generated (not planted) projected values: no scaled mantissa within 1e-3 of where the rounding rule
    switches (x.5 to nearest, an integer under truncation), no |y| within 1 % of atol."""
    y = np.asarray(y, dtype=np.float64)
    t = np.abs(scaled_mantissa(y, scale))
    frac = t - np.floor(t)
    tie = np.abs(frac - 0.5) if scale > 0 else np.minimum(frac, 1.0 - frac)
    away = np.abs(np.abs(y) - atol) >= 0.01 * atol
    return ((tie >= 1e-3) | (np.abs(y) < atol)) & away  # (below atol the mantissa is never looked at)


# what the entries of every generated channel source hold somewhere: INT32_MIN and its neighbour, INT32_MAX; the largest integers a float
# channel may hold (|v| < 2^24)
CHAN_EXTREMES = {np.int32: (INT32_MIN, 2 ** 31 - 1, INT32_MIN + 1), np.float32: (2 ** 24 - 1, -(2 ** 24) + 1)}


def _chan_pool(rng, dtype, size):
    if dtype == np.float32:
        v = rng.integers(-(2 ** 24) + 1, 2 ** 24, size=size)
        v.flat[:4] = [2 ** 24 - 1, -(2 ** 24) + 1, -1, 1][:min(4, v.size)]
        return v
    v = rng.integers(INT32_MIN, 2 ** 31, size=size)
    v.flat[:5] = [INT32_MIN, 2 ** 31 - 1, -1, 1, INT32_MIN + 1][:min(5, v.size)]
    return v


def make_case(kind, n, T=0, r=0, packed=1, lab_packed=1, seed=0, classes=34, subs=3, atol=ATOL, key=KEY, round_mode="nearest"):
    """A source of `kind` whose old labels (0 .. classes, canonical, with a label-0 region) are refined by `subs` variants of the
    projected value and of the channel values per old class; variant 0 of the labels 0 and 1 is "all zero": the zero class, and a
    class (1, 0 ..) that differs from it in the label alone.  subs = 1: the new partition is the old one.  Noise wherever no kernel may read: the padding
    of C, and the strict upper triangle of C, U, a, b and of full labels under a packed source."""
    rng = np.random.default_rng(seed)
    ii, jj = entries(n, packed)
    nent = len(ii)
    ld = -(-n // 128) * 128
    case = dict(kind=kind, n=n, ld=ld, T=T, r=r, packed=packed, lab_packed=lab_packed, atol=atol, key=key, round_mode=round_mode)
    scale = round_scale(atol, round_mode)
    if kind == "pair":
        assert lab_packed == packed
        groups = classes + 1
        g = np.concatenate([np.arange(groups), rng.integers(0, groups, size=nent - groups)]) if nent >= groups else rng.integers(0, groups, size=nent)
        g = g[rng.permutation(nent)]
        one = 0.7431
        # +-0, two values one bit apart, a subnormal; group 0 is (+0, +0), then (+0, -0), .. (-0, +0), (-0, -0), .. row by row
        va_pool = np.concatenate([[0.0, -0.0, one, np.nextafter(one, 2.0), -one, 3.0e-310, 1.5], rng.standard_normal(max(0, classes // 5))])
        vb_pool = np.array([0.0, -0.0, 2.5, np.nextafter(2.5, 0.0), -2.5])
        pairs = [(x, y) for x in range(len(va_pool)) for y in range(len(vb_pool))]
        assert len(pairs) >= groups
        pick = pairs[:groups]
        va, vb = np.array([va_pool[p[0]] for p in pick]), np.array([vb_pool[p[1]] for p in pick])
        a, b = np.full(n * n, np.nan), np.full(n * n, np.nan)  # NaN: nobody may read the strict upper triangle
        ef = jj * n + ii if packed else np.arange(n * n)
        a[ef], b[ef] = va[g], vb[g]
        case.update(a=a, b=b, L=np.full(nent, 0xDEAD, dtype=np.uint32))
        return case
    lold = _canonical_old_labels(rng, nent, classes)
    sub = rng.integers(0, subs, size=nent)  # the variant of the channel values ...
    sub_u = rng.integers(0, subs, size=nent) if kind == "joint" else sub  # ... and, drawn apart from it, of the projected value
    sub[np.flatnonzero(lold == 0)[-1]] = sub_u[np.flatnonzero(lold == 0)[-1]] = 0  # (a zero class at any size)
    if kind in ("proj", "joint"):
        coef = rng.integers(1, 64, size=r) * rng.choice([-1.0, 1.0], size=r) / 64.0
        tab = rng.integers(-1023, 1024, size=(r, classes + 1, subs)) / 1024.0
        tab[:, :2, 0] = 0.0
        x = class_uniform(key, np.arange(classes + 1))
        for _ in range(200):  # redraw the variants whose projected value sits inside a margin
            y = x[:, None] - np.tensordot(coef, tab, axes=1) if r else np.broadcast_to(x[:, None], (classes + 1, subs))
            bad = ~_margins_ok(y, atol, scale)
            bad[:2, 0] = False
            if not bad.any() or r == 0:
                break
            tab[:, bad] = rng.integers(-1023, 1024, size=(r, int(bad.sum()))) / 1024.0
        U = rng.integers(-1023, 1024, size=r * n * n) / 1024.0  # noise where nothing is set below
        ef = jj * n + ii
        for k in range(r):
            U[k * n * n + ef] = tab[k, lold, sub_u]
        check_exact_projection(U, coef)
        case.update(U=U, coef=coef)
    if kind != "proj":
        dtype = np.float32 if kind == "chan_f32" else np.int32
        ctab = _chan_pool(rng, dtype, (T, classes + 1, subs))
        ctab[:, :2, 0] = 0
        if subs > 1:  # variants that differ in ONE channel only, each channel in turn
            for t in range(T):
                ctab[:, 1 + t % classes, 1] = ctab[:, 1 + t % classes, subs - 1]
                ctab[t, 1 + t % classes, 1] ^= 1 if dtype == np.int32 else 2
        # the extremes of the number format, planted last -- behind the zeroing and the one-channel variants -- into (label, variant)
        # slots that entries do take, one channel each; the classes of the one-channel variants are left alone where others exist
        slots = sorted({(int(l), int(v)) for l, v in zip(lold, sub) if not (l < 2 and v == 0)})
        free = [q for q in slots if subs == 1 or q[0] == 0 or q[0] > min(T, classes)] or slots
        cells = [(t, l, q) for l, q in free for t in range(T)]
        ext = CHAN_EXTREMES[dtype][:len(cells)]  # (a cell each: all of them wherever three cells exist)
        for k, v in enumerate(ext):
            ctab[cells[k * (len(cells) // len(ext))]] = v
        C = _chan_pool(rng, dtype, T * ld * ld).astype(dtype)
        for t in range(T):
            C[t * ld * ld + jj * ld + ii] = ctab[t, lold, sub]
        read = np.concatenate([C[t * ld * ld + jj * ld + ii] for t in range(T)]).astype(np.int64)
        assert len(ext) >= 1 and all(v in read for v in ext), "an extreme value no kernel would read"
        case.update(C=C)
    if lab_packed or not packed:
        L = lold.astype(np.uint32)
    else:
        L = rng.integers(0, classes + 1, size=n * n).astype(np.uint32)  # noise in the strict upper triangle
        L[jj * n + ii] = lold
    case.update(L=L)
    if kind in ("proj", "joint"):
        assert _margins_ok(projected(case), atol, scale).all()
    return case


def make_count_case(kind, n, nclasses, seed=0, packed=1, lab_packed=1, T=2, r=1, distinct_in=0, dense_chunk=0, last_alone=False, classes=34,
                    atol=ATOL, key=KEY):
    """chan_i32 / joint / pair source with exactly `nclasses` new classes besides the zero class: new class g has the old label
    1 + g % classes and channel 0 = a value of its own (pair: a = a value of its own).  distinct_in = k: the entries of the old
    classes 1 .. k get a channel-0 value each instead (about len k / classes more classes).  dense_chunk = m: the first 2048
    entries hold m classes of their own, each several times.  last_alone: the last entry is the only one of its class."""
    rng = np.random.default_rng(seed)
    ii, jj = entries(n, packed)
    nent = len(ii)
    ld = -(-n // 128) * 128
    used = nclasses - 1 if last_alone else nclasses
    body_classes = np.arange(dense_chunk, used)  # (the classes below dense_chunk live in the first 2048 entries only)
    nbody = nent - 1 - (2048 if dense_chunk else 0)
    assert nbody >= 2 * len(body_classes) + 64
    body = np.concatenate([body_classes, body_classes, np.full(64, -1), rng.choice(body_classes, size=nbody - 2 * len(body_classes) - 64)])
    head = rng.permutation(np.arange(2048) % dense_chunk) if dense_chunk else np.zeros(0, dtype=np.int64)
    g = np.concatenate([head, body[rng.permutation(nbody)], [used if last_alone else body_classes[0]]]).astype(np.int64)
    zero = g < 0  # 64 entries of the zero class
    g = np.where(zero, 0, g)
    case = dict(kind=kind, n=n, ld=ld, T=T, r=r, packed=packed, lab_packed=lab_packed, atol=atol, key=key, round_mode="nearest")
    val = rng.permutation(2 ** 20)[:nclasses] - 2 ** 19  # a value per class, none twice
    val[val == 0] = 2 ** 19
    if kind == "pair":
        a, b = np.full(n * n, np.nan), np.full(n * n, np.nan)
        ef = jj * n + ii if packed else np.arange(n * n)
        a[ef] = np.where(zero, 0.0, val[g] / 1024.0)
        b[ef] = np.where(zero, 0.0, (g % 3) * 0.5)
        case.update(a=a, b=b, L=np.full(nent, 0xDEAD, dtype=np.uint32))
        return case
    lold = np.where(zero, 0, 1 + g % classes)
    c0 = np.where(zero, 0, val[g])
    if distinct_in:
        sel = (lold >= 1) & (lold <= distinct_in)
        c0 = np.where(sel, 2 ** 21 + np.arange(nent), c0)
    C = rng.integers(INT32_MIN, 2 ** 31, size=T * ld * ld).astype(np.int32)
    C[jj * ld + ii] = c0
    for t in range(1, T):
        C[t * ld * ld + jj * ld + ii] = np.where(zero, 0, np.array([3, -7 * t, INT32_MIN, 2 ** 31 - 1, -1])[lold % 5])  # (a function of the old label)
    case.update(C=C)
    if kind == "joint":
        coef = np.full(r, 0.5)
        utab = rng.integers(-1023, 1024, size=(r, classes + 1)) / 1024.0
        for _ in range(200):  # (redraw the labels whose projected value sits inside a margin)
            utab[:, 0] = 0.0
            bad = ~_margins_ok(class_uniform(key, np.arange(classes + 1)) - coef @ utab, atol, round_scale(atol))
            if not bad[1:].any():
                break
            utab[:, bad] = rng.integers(-1023, 1024, size=(r, int(bad.sum()))) / 1024.0
        assert not bad.any()
        U = rng.integers(-1023, 1024, size=r * n * n) / 1024.0
        for k in range(r):
            U[k * n * n + jj * n + ii] = utab[k, lold]
        check_exact_projection(U, coef)
        case.update(U=U, coef=coef)
    if lab_packed or not packed:
        L = lold.astype(np.uint32)
    else:
        L = rng.integers(0, classes + 1, size=n * n).astype(np.uint32)
        L[jj * n + ii] = lold
    case.update(L=L)
    return case


# targets of the planted projected values: atol itself, the double below it, a mantissa that rounds up to 1.0 beside the power of
# two it folds onto (to nearest; truncation keeps them apart), and the truncation edge 0.0625 with a neighbour just below it
PLANTS = (ATOL, np.nextafter(ATOL, 0.0), 0.25, 0.25 - 2.0 ** -32, -(0.25 - 2.0 ** -32), 0.0625, 0.0625 - 2.0 ** -40, 0.5 - 2.0 ** -30)
TINY_LABEL = 5  # under planted_key(), class 5 draws x = m 2^-53 < 2^-27: x - (the double below atol) fits 53 bits
_PLANTED = []


def planted_key(classes=9):
    """(key, m): the first m >= 3 * 2^13 whose key draws x(TINY_LABEL) = m 2^-53 and, for the other labels up to `classes`, values that
    keep the generator's margins under both rounding rules (an unplanted entry's projected value is x(l) itself)."""
    if not _PLANTED:
        for m in range(3 << 13, (3 << 13) + 4096):
            key = key_with_uniform(TINY_LABEL, m)
            x = class_uniform(key, np.arange(1, classes + 1))
            if _margins_ok(x, ATOL, 1e7).all() and _margins_ok(x, ATOL, -1e7).all():
                _PLANTED.append((key, m))
                break
    return _PLANTED[0]


def make_planted_case(kind, n, round_mode, T=2, packed=1, lab_packed=1, seed=0, classes=9):
    """r = 1, coef = 1, U[e] = x(l) - target: the projected value IS the target, exactly.  Every target once under label 0 (where x = 0),
    once under TINY_LABEL and under every other label l for which x(l) - (x(l) - target) == target in float64; elsewhere U = 0 (y = x(l))."""
    key, tiny_m = planted_key()
    assert classes <= 9
    case = make_case(kind, n, T=T, r=1, packed=packed, lab_packed=lab_packed, seed=seed, classes=classes, subs=1, key=key, round_mode=round_mode)
    ii, jj = entries(n, packed)
    lold = old_labels(case).astype(np.int64)
    x = class_uniform(key, lold)
    assert x[lold == TINY_LABEL][0] == tiny_m * 2.0 ** -53 < 2.0 ** -27
    case["coef"] = np.array([1.0])
    U = case["U"]
    U[jj * n + ii] = 0.0
    rng = np.random.default_rng(seed + 1)
    planted = np.zeros(len(ii), dtype=bool)
    for ti, target in enumerate(PLANTS):
        for l in range(classes + 1):
            xl = class_uniform(key, np.array([l]))[0]
            if xl - (xl - target) != target:  # x(l) - target needs more than 53 bits: no u gives this target under this label
                assert l not in (0, TINY_LABEL)
                continue
            cand = np.flatnonzero((lold == l) & ~planted)
            for e in rng.permutation(cand)[:2]:  # twice: the planted entries of one (label, target) share a class
                u = x[e] - target
                assert x[e] - u == target  # exact both ways
                U[jj[e] * n + ii[e]] = u
                planted[e] = True
    case["planted"] = planted
    y = projected(case)
    assert _margins_ok(y[~planted], case["atol"], round_scale(case["atol"], round_mode)).all()
    return case
