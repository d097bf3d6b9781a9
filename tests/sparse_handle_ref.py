"""A plain sequential restatement of the canonical CSR form of a sparse-constraints handle (``sdpsr_sparse_create``) and of
its symmetry predicate, and the cases the handle's tests run on.

The canonical form is the one ``canonicalize_csr`` defines (csrc/setup_csr.cpp): each row sorted by column with a stable
sort, duplicates summed left to right in input order (``s = v0; s += v1; ...`` -- a Python loop here, never
``np.add.reduceat``, which may sum runs of 8 or more pairwise), every ``v == 0.0`` of either sign dropped.
"""
import numpy as np


def canonical(len_, rowptr, colind, val, base=0):
    """(rowptr, colind, val) canonical and 0-based -- int64, int64, float64 -- or ValueError with the library's message."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colind = np.asarray(colind, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    if base not in (0, 1):
        raise ValueError("index_base must be 0 or 1")
    m = rowptr.size - 1
    if m == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    if rowptr[0] != base:
        raise ValueError("rowptr[0] != index_base")
    for i in range(m):
        if rowptr[i + 1] < rowptr[i]:
            raise ValueError(f"rowptr is not monotone at row {i}")
    nnz = int(rowptr[m] - base)
    if nnz != colind.size:
        raise ValueError("rowptr[m] - index_base != nnz")
    for p in range(nnz):
        k = int(colind[p]) - base
        if k < 0 or k >= len_:
            raise ValueError(f"column index out of [0, n^2) at entry {p}")
        if not np.isfinite(val[p]):
            raise ValueError(f"non-finite value at entry {p}")
    out_rp, out_c, out_v = [0], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(m):
            a, b = int(rowptr[i]) - base, int(rowptr[i + 1]) - base
            order = sorted(range(a, b), key=lambda p: int(colind[p]))  # (sorted is stable)
            q = 0
            while q < len(order):
                k = int(colind[order[q]])
                s = np.float64(val[order[q]])
                t = q + 1
                while t < len(order) and int(colind[order[t]]) == k:
                    s = s + np.float64(val[order[t]])
                    t += 1
                if not np.isfinite(s):
                    raise ValueError("duplicate entries sum to a non-finite value")
                if s != 0.0:
                    out_c.append(k - base)
                    out_v.append(s)
                q = t
            out_rp.append(len(out_c))
    return np.array(out_rp, dtype=np.int64), np.array(out_c, dtype=np.int64), np.array(out_v, dtype=np.float64)


def rows_symmetric(len_, rowptr, colind, val):
    """The predicate of ``csr_rows_symmetric`` on canonical 0-based arrays: ``len_`` is a perfect square n^2 and every row is
    a symmetric n x n matrix bit for bit."""
    n = int(np.floor(np.sqrt(len_)))
    while n * n > len_:
        n -= 1
    while (n + 1) * (n + 1) <= len_:
        n += 1
    if n * n != len_:
        return False
    bits = np.asarray(val, dtype=np.float64).view(np.uint64)
    for i in range(len(rowptr) - 1):
        a, b = int(rowptr[i]), int(rowptr[i + 1])
        row = {int(colind[p]): int(bits[p]) for p in range(a, b)}
        for k, v in row.items():
            r, q = k % n, k // n
            if r != q and row.get(q + r * n) != v:
                return False
    return True


def max_run(rowptr, colind, base=0):
    """The longest run of duplicates (equal column inside one row) of raw arrays."""
    best = 0
    for i in range(len(rowptr) - 1):
        cols = np.asarray(colind[int(rowptr[i]) - base:int(rowptr[i + 1]) - base])
        if cols.size:
            best = max(best, int(np.unique(cols, return_counts=True)[1].max()))
    return best


def bits_equal(a, b):
    """Two canonical triples agree bit for bit (-0.0 and NaN payloads count)."""
    return (len(a) == len(b) == 3 and np.array_equal(np.asarray(a[0], dtype=np.int64), np.asarray(b[0], dtype=np.int64))
            and np.array_equal(np.asarray(a[1], dtype=np.int64), np.asarray(b[1], dtype=np.int64))
            and np.array_equal(np.ascontiguousarray(a[2], dtype=np.float64).view(np.uint64),
                               np.ascontiguousarray(b[2], dtype=np.float64).view(np.uint64)))


def _csr(rows):
    """rows: per row a list of (column, value) in input order."""
    rp, ci, va = [0], [], []
    for row in rows:
        for k, v in row:
            ci.append(k)
            va.append(v)
        rp.append(len(ci))
    return np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int64), np.array(va, dtype=np.float64)


def scan_case():
    """nnz = 3 * 2048 + 17 raw entries over m = 4 rows at len = 48^2: duplicates and zeros on both sides of every boundary of
    the compaction's 2048-entry chunks, one row boundary inside a chunk, shuffled rows (more than one sort block)."""
    rng = np.random.default_rng(2048)
    len_, nnz = 48 * 48, 3 * 2048 + 17
    bounds = [0, 2048 - 3, 2048 + 1000, 2 * 2048 + 5, nnz]  # rows 0 | 1 | 2 | 3; the boundary 3048 lies inside chunk 1
    rows = []
    for i in range(4):
        cnt = bounds[i + 1] - bounds[i]
        cols = rng.integers(0, len_, size=cnt)
        vals = rng.integers(-3, 4, size=cnt).astype(np.float64)  # zeros, and duplicates that cancel
        rows.append([[int(k), float(v)] for k, v in zip(cols, vals)])
    flat = [e for row in rows for e in row]
    for cb in (2048, 4096, 6144):  # around every chunk boundary: a duplicate pair, an explicit zero, a cancelling pair
        for off, v in ((-4, 2.5), (-3, 0.0), (-2, 1.5), (-1, -1.5), (0, 0.0), (1, 2.5), (2, -0.0), (3, 0.75)):
            flat[cb + off][1] = v
        flat[cb - 3][0] = flat[cb - 4][0]
        flat[cb - 1][0] = flat[cb - 2][0]
        flat[cb + 1][0] = flat[cb][0]
    return len_, _csr([[tuple(e) for e in row] for row in rows])


def canonical_cases():
    """name -> (len_, (rowptr, colind, val)), all 0-based."""
    rng = np.random.default_rng(7)
    cases = {}
    sorted_rows = [[(0, 1.0), (3, -2.0), (7, 0.5), (15, 4.0)], [(1, 1.5), (2, 2.5)], [(5, -1.0), (6, 3.0), (9, 1e-300)]]
    cases["sorted"] = (16, _csr(sorted_rows))
    swapped = [list(r) for r in sorted_rows]
    swapped[1] = swapped[1][::-1]  # one swapped pair: the sort route on the same matrix
    cases["one_swapped_pair"] = (16, _csr(swapped))
    shuffled = [[r[j] for j in rng.permutation(len(r))] for r in sorted_rows]
    cases["shuffled"] = (16, _csr(shuffled))
    cases["empty_rows_sorted"] = (16, _csr([[], [(2, 1.0), (4, 2.0)], [], [], [(1, 3.0)], []]))
    cases["empty_rows_shuffled"] = (16, _csr([[], [(4, 2.0), (2, 1.0)], [], [], [(1, 3.0), (1, 1.0)], []]))
    cases["m0"] = (16, _csr([]))
    cases["nnz0"] = (16, _csr([[], [], []]))
    cases["explicit_zeros_sorted"] = (16, _csr([[(0, 0.0), (1, 1.0), (2, -0.0)], [(3, -0.0)], [(4, 2.0), (5, 0.0)]]))
    cases["explicit_zeros_shuffled"] = (16, _csr([[(2, -0.0), (1, 1.0), (0, 0.0)], [(3, -0.0)], [(5, 0.0), (4, 2.0)]]))
    cases["cancelling_duplicates"] = (16, _csr([[(3, 1.5), (1, 2.0), (3, -1.5)], [(2, 0.25), (2, -0.25)], [(7, 1.0), (7, 1.0)]]))
    # the order of the additions decides: [1e16, -1e16, 1.0] keeps 1.0; [1.0, 1e16, -1e16] sums to 0 and is dropped
    cases["order_sensitive"] = (16, _csr([[(4, 1e16), (9, 1.0), (4, -1e16), (9, 1e16), (4, 1.0), (9, -1e16)], [(0, 1.0)], []]))
    run = [(5, float(v)) for v in np.ldexp(rng.standard_normal(40), rng.integers(-30, 30, size=40))]
    cases["run_of_40"] = (16, _csr([[(1, 1.0)] + run[:20] + [(0, 2.0)] + run[20:], [(5, 1.0)], []]))
    cases["scan"] = scan_case()
    return cases


def _sym_rows(n, rng, rows=2, pairs=4):
    out = []
    for _ in range(rows):
        row = {}
        for _ in range(pairs):
            i, j = (int(x) for x in rng.integers(0, n, size=2))
            v = float(rng.standard_normal())
            row[i + j * n] = v
            row[j + i * n] = v
        out.append(sorted(row.items()))
    return out


def symmetry_cases():
    """name -> (len_, (rowptr, colind, val), expected rows_symmetric)."""
    cases = {}
    for n in (4, 7):
        rng = np.random.default_rng(n)
        base_rows = _sym_rows(n, rng)
        cases[f"symmetric_n{n}"] = (n * n, _csr(base_rows), True)
        k, v = next((k, v) for k, v in base_rows[1] if k % n != k // n)
        t = (k // n) + (k % n) * n
        bit = [list(r) for r in base_rows]
        bit[1] = [(kk, float(np.nextafter(vv, np.inf)) if kk == t else vv) for kk, vv in bit[1]]
        cases[f"last_bit_n{n}"] = (n * n, _csr(bit), False)
        miss = [list(r) for r in base_rows]
        miss[1] = [(kk, vv) for kk, vv in miss[1] if kk != t]
        cases[f"missing_transpose_n{n}"] = (n * n, _csr(miss), False)
        cases[f"diagonal_only_n{n}"] = (n * n, _csr([[(i + i * n, float(i + 1)) for i in range(n)], [(0, 2.0)]]), True)
        # symmetric only once the duplicates are summed: (1, 2) = 0.5 + 0.25, (2, 1) = 0.75
        cases[f"symmetric_after_sum_n{n}"] = (n * n, _csr([[(1 + 2 * n, 0.5), (2 + 1 * n, 0.75), (1 + 2 * n, 0.25)], [(0, 1.0)]]), True)
        # the predicate looks at the CANONICAL row: both positions are stored before the zeros are dropped (a symmetric
        # pattern), but (1, 3) = 1 - 1 is dropped and (3, 1) = 1 stays without its partner; and a pair 0.0 / -0.0, whose
        # bits differ while they are stored, is dropped on both sides and leaves a symmetric row
        cases[f"asymmetric_after_drop_n{n}"] = (n * n, _csr([[(1 + 3 * n, 1.0), (3 + 1 * n, 1.0), (1 + 3 * n, -1.0)], [(0, 1.0)]]), False)
        cases[f"negative_zero_pair_n{n}"] = (n * n, _csr([[(1 + 3 * n, 0.0), (3 + 1 * n, -0.0), (2 + 2 * n, 1.0)]]), True)
    cases["non_square_len"] = (15, _csr([[(0, 1.0)], [(7, 2.0)]]), False)
    return cases
