"""NumPy restatement of the reduced PSD pencil from triplets (sdpsr_blockop_*): Z_k(x) = sum_i x_i blks[i][k] and its adjoint
g_i = sum_k <blks[i][k], S_k>.  tests/test_blockop_cpu.py checks it on its own, tests/test_gpu_blockop.py compares the library
with it.  No dependence on the library.

A POSITION is the flat index of (block, row, col) in the one-class layout of sdpsr_block_images: blocks side by side, each
column-major.  The FULL entry list: every triplet, and under `upper` a mirror (col, row) right behind each triplet with
row != col.  Every sum is taken in float64, term by term in list order; `c` counts the terms of an output element and `mag`
is the sum of their absolute values -- the two figures of the bound |err| <= (c + 2) eps mag of a sum of c products in any
order."""
import numpy as np

EPS = np.finfo(np.float64).eps


def block_offsets(sizes):
    return np.concatenate([[0], np.cumsum([int(s) ** 2 for s in sizes])]).astype(np.int64)


def full_entries(classptr, blk, row, col, val, sizes, upper=True, index_base=0):
    """(cls, pos, val) of the full entry list, class-major in input order, a mirror right behind its entry."""
    classptr = np.asarray(classptr, dtype=np.int64)
    b, r, c = (np.asarray(a, dtype=np.int64) - index_base for a in (blk, row, col))
    v = np.asarray(val, dtype=np.float64)
    cls = np.repeat(np.arange(classptr.size - 1, dtype=np.int64), np.diff(classptr))
    off, s = block_offsets(sizes), np.asarray(sizes, dtype=np.int64)
    pos = off[b] + r + c * s[b]
    if not upper:
        return cls, pos, v
    mpos = off[b] + c + r * s[b]
    reps = 1 + (r != c).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(reps)[:-1]]).astype(np.int64)
    fpos = np.repeat(pos, reps)
    fpos[first[reps == 2] + 1] = mpos[reps == 2]
    return np.repeat(cls, reps), fpos, np.repeat(v, reps)


def _keyed(key, terms, n):
    out, mag = np.zeros(n), np.zeros(n)
    with np.errstate(invalid="ignore"):
        np.add.at(out, key, terms)
        np.add.at(mag, key, np.abs(terms))
    return out, np.bincount(key, minlength=n).astype(np.int64), mag


def apply_ref(x, full, sum_sq):
    """(Z, c, mag): Z[p] = sum x[cls] * val over the full entries at position p."""
    cls, pos, v = full
    return _keyed(pos, np.asarray(x, dtype=np.float64)[cls] * v, int(sum_sq))


def adjoint_ref(S, full, d):
    """(g, c, mag): g[i] = sum val * S[pos] over the full entries of class i."""
    cls, pos, v = full
    return _keyed(cls, v * np.asarray(S, dtype=np.float64)[pos], int(d))


def split_blocks(flat, sizes):
    off = block_offsets(sizes)
    return [np.asarray(flat)[off[k]:off[k + 1]].reshape(int(s), int(s), order="F") for k, s in enumerate(sizes)]


def flatten_blocks(blocks):
    return np.concatenate([np.asarray(b, dtype=np.float64).ravel(order="F") for b in blocks])


def random_triplets(sizes, d, density, seed, upper=True, index_base=0, empty_class=None, empty_block=None, zero_pos=None):
    """Seeded triplets in scan order (class, block, column-major): a share `density` of the positions of every class.
    empty_class / empty_block: no entry there; zero_pos = (block, row, col): no class touches that position (or its mirror)."""
    rng = np.random.default_rng(seed)
    ptr, bk, rr, cc, vv = [0], [], [], [], []
    for i in range(d):
        for k, s in enumerate(sizes):
            for c in range(s):
                for r in range(s):
                    if upper and r > c:
                        continue
                    keep = rng.random() < density
                    v = rng.standard_normal()
                    if i == empty_class or k == empty_block or not keep:
                        continue
                    if zero_pos is not None and k == zero_pos[0] and {r, c} == {zero_pos[1], zero_pos[2]}:
                        continue
                    bk.append(k), rr.append(r), cc.append(c), vv.append(v)
        ptr.append(len(bk))
    ib = index_base
    return (np.asarray(ptr, dtype=np.int64), np.asarray(bk, dtype=np.int32) + ib, np.asarray(rr, dtype=np.int32) + ib,
            np.asarray(cc, dtype=np.int32) + ib, np.asarray(vv, dtype=np.float64))
