"""Python side of the square check (csrc/kernels_square_check.hip): integer mirrors of the hash rules it shares with the host
(csrc/sdpsr_hash.h), the EXACT answer to the question it asks, the values its kernels must store, and the inputs of
tests/test_gpu_square_check.py and tests/test_square_check_ref_cpu.py.

The question, per round (key) and channel t: with X_t[i, j] = the int8 value of class L[i, j] (0 on label 0), does X_t @ X_t take
on every entry the value it takes at the representative of the entry's class, and 0 on label 0?  The check answers it with one
random vector v per round: c[k] = (X_t @ X_t)[representative of class k], y = X_t v, w = C v with C[i, j] = c[L[i, j]], and
"equal" exactly when sum(y_i^2) == sum(v_i w_i)."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
VKEY = 0xA24BAED4963EE407
KEYS = (0x0123456789ABCDEF, 0x0FEDCBA987654321)  # the two rounds of every test


def fmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def class_bits(key, label):
    return fmix64((key + GOLD * label) & M64)


def class_i8(bits, t):
    b = (bits >> (8 * t)) & 0xFF
    return b - 256 if b >= 128 else b


def check_vector_key(key):
    return fmix64(key ^ VKEY)


def check_vector(kv, i):
    return (class_bits(kv, i + 1) >> 48) & 0xFFFF


def col_off(n, j):
    return j * n - j * (j - 1) // 2


def packed_ij(n):
    cols = np.arange(n)
    return np.concatenate([np.arange(j, n) for j in range(n)]), np.repeat(cols, n - cols)


def pack(L):
    ii, jj = packed_ij(L.shape[0])
    return np.ascontiguousarray(L[ii, jj].astype(np.uint32))


def first_of(L):
    """Packed index of the first entry of every label 1 .. max(L) (all present)."""
    Lp = pack(L)
    d = int(Lp.max())
    first = np.full(d + 1, -1, dtype=np.int64)
    idx = np.arange(len(Lp))[::-1]
    first[Lp[::-1]] = idx
    assert (first[1:] >= 0).all()
    return first[1:].astype(np.uint32)


def class_tables(key, d, T):
    """[T][d + 1] int64: the channel values of labels 0 .. d (0 for label 0)."""
    tab = np.zeros((T, d + 1), dtype=np.int64)
    for l in range(1, d + 1):
        b = class_bits(key, l)
        for t in range(T):
            tab[t, l] = class_i8(b & 0xFFFFFFFF, t)
    return tab


def vector(key, n):
    kv = check_vector_key(key)
    return np.array([check_vector(kv, i) for i in range(n)], dtype=np.int64)


def reference(L, first, key, T):
    """Everything about one round: exact[t] (the true answer), c [T][d], y, w [T][n] (int64), q1, q2 [T] (Python integers) and
    equal[t] = (q1 == q2)."""
    n, d = L.shape[0], len(first)
    ii, jj = packed_ij(n)
    ri, rj = ii[first.astype(np.int64)], jj[first.astype(np.int64)]
    tab = class_tables(key, d, T)
    v = vector(key, n)
    out = {"exact": [], "c": np.zeros((T, d), dtype=np.int64), "y": np.zeros((T, n), dtype=np.int64), "w": np.zeros((T, n), dtype=np.int64),
           "q1": [], "q2": [], "equal": []}
    for t in range(T):
        X = tab[t][L]
        S = (X.astype(np.float64) @ X.astype(np.float64)).astype(np.int64)  # |entries| <= 2^14 n: exact in float64
        c = S[ri, rj]
        Cm = np.concatenate([[0], c])[L]
        y, w = X @ v, Cm @ v
        q1 = sum(int(a) * int(a) for a in y)
        q2 = sum(int(a) * int(b) for a, b in zip(v, w))
        out["exact"].append(bool(np.array_equal(S, Cm)))
        out["c"][t], out["y"][t], out["w"][t] = c, y, w
        out["q1"].append(q1), out["q2"].append(q2), out["equal"].append(q1 == q2)
    return out


# the names build_cases gives its inputs, in order (the GPU test is parametrised by them)
NAMES = ("circ256", "jordan64", "jordan512", "er7xk1", "er7xk2", "er7xk9", "direct_sum_zero_block", "one_entry", "ones63", "complete64", "complete65",
         "circ67_d34", "circ130", "circ257", "circ509_d255", "random63_d34", "random65_d255", "random130_d2", "random257_d34", "random513_d255",
         "random513_d1", "merged130", "needle_first_tile", "needle_last_tile", "needle_diagonal_tile", "needle_offdiagonal_tile", "needle_last_row_odd",
         "zero_over_nonzero", "wrong_representative")

_cache = {}


def reference_of(case, g):
    """The T = 4 reference of round g of a case (T = 2: its first two channels), computed once."""
    k = (case["name"], g)
    if k not in _cache:
        _cache[k] = reference(case["L"], case["first"], KEYS[g], 4)
    return _cache[k]


def _renumber(L):
    """Labels 1 .. d without holes, 0 kept (any order: the check does not care how classes are numbered)."""
    u = np.unique(L)
    m = np.zeros(int(u.max()) + 1, dtype=np.int64)
    m[u[u != 0]] = np.arange(1, (u != 0).sum() + 1)
    return m[L]


def _random_labels(n, d, with_zero, seed):
    rng = np.random.default_rng(seed)
    npk = n * (n + 1) // 2
    d = max(1, min(d, npk - (1 if with_zero and npk > 1 else 0)))
    g = np.concatenate([np.arange(1, d + 1), rng.integers(0 if with_zero else 1, d + 1, size=npk - d)])
    g = g[rng.permutation(npk)]
    ii, jj = packed_ij(n)
    L = np.zeros((n, n), dtype=np.int64)
    L[ii, jj] = g
    L[jj, ii] = g
    return L


def _needle(L, i, j):
    """Entry (i, j) and its mirror moved to another class that stays non-empty either way."""
    L = L.copy()
    d = int(L.max())
    new = L[i, j] % d + 1
    assert new != L[i, j] and (L == L[i, j]).sum() > 2
    L[i, j] = L[j, i] = new
    return L


def build_cases(problems, golden):
    """name, L (symmetric n x n int64, labels 0 .. d), first (d packed indices), closed (the expected exact answer, or None: whatever it is)."""
    P = problems
    cases = []

    def add(name, L, closed, first=None):
        L = np.ascontiguousarray(np.asarray(L, dtype=np.int64))
        assert np.array_equal(L, L.T) and L.max() <= 255
        cases.append({"name": name, "L": L, "first": first_of(L) if first is None else first, "closed": closed})

    # closed inputs
    add("circ256", golden["circ256_P"], True)
    add("jordan64", P.synthetic_jordan_partition(64, seed=3)[0], True)
    add("jordan512", P.synthetic_jordan_partition(512, seed=3)[0], True)
    for k in (1, 2, 9):
        add("er7xk%d" % k, P.kron_with_complete(golden["er7_P"], k, seed=2)[0], True)
    add("direct_sum_zero_block", P.direct_sum_labels([(2, 3), (3, 2)]), True)
    add("one_entry", np.ones((1, 1)), True)                    # n = 1, d = 1
    add("ones63", P.ones_labels(63), True)                     # d = 1, below a tile edge
    add("complete64", P.complete_scheme_labels(64), True)      # d = 2, one tile
    add("complete65", P.complete_scheme_labels(65), True)      # d = 2, a row and a column of a second tile
    add("circ67_d34", P.symmetric_circulant_labels(67), True)  # d = 34
    add("circ130", P.symmetric_circulant_labels(130), True)
    add("circ257", P.symmetric_circulant_labels(257), True)
    add("circ509_d255", P.symmetric_circulant_labels(509), True)  # d = 255
    # made-up labels of every order and class count: whatever the answer, every stored value must be the reference's
    for n, d, z in ((63, 34, True), (65, 255, False), (130, 2, True), (257, 34, False), (513, 255, True), (513, 1, True)):
        add("random%d_d%d" % (n, d), _random_labels(n, d, z, seed=n + d), None)
    # not closed
    c130, c257, c64 = P.symmetric_circulant_labels(130), P.symmetric_circulant_labels(257), P.symmetric_circulant_labels(64)
    merged = c130.copy()
    merged[merged == 3] = 2
    add("merged130", _renumber(merged), False)
    add("needle_first_tile", _needle(c130, 5, 3), False)
    add("needle_last_tile", _needle(c130, 129, 128), False)
    add("needle_diagonal_tile", _needle(c130, 100, 70), False)
    add("needle_offdiagonal_tile", _needle(c130, 129, 3), False)
    add("needle_last_row_odd", _needle(c257, 256, 100), False)
    zero = c64.copy()
    zero[zero == 3] = 0
    add("zero_over_nonzero", _renumber(zero), False)
    wrong = first_of(c130)
    wrong[4] = wrong[7]  # class 5 is judged by an entry of class 8
    add("wrong_representative", c130, False, first=wrong)
    assert tuple(c["name"] for c in cases) == NAMES
    return cases
