"""NumPy restatement of sdpsr_block_images_sparse (tests/test_sparse_images_cpu.py checks it, tests/test_gpu_sparse_images.py
compares the library with it, exactly).  No dependence on the library.

Input: ``flat``, class_count * sum s_k^2 elements (float64 or complex128), class-major, then block, each block column-major --
the layout of sdpsr_block_images.  The virtual block is the block itself, or for complex input its real embedding
[Re -Im; Im Re] of order 2 s_k.  Kept: !(|v| <= tol).  Order: class, block, column-major inside the block."""
import numpy as np


def embed(Z):
    """[Re -Im; Im Re] of the last two axes."""
    Z = np.asarray(Z)
    return np.concatenate([np.concatenate([Z.real, -Z.imag], axis=-1), np.concatenate([Z.imag, Z.real], axis=-1)], axis=-2)


def virtual_sizes(sizes, is_complex):
    return [2 * int(s) if is_complex else int(s) for s in sizes]


def virtual_blocks(flat, sizes):
    """vb[k][i] = virtual block k of class i as an (s'_k, s'_k) matrix indexed [row, col]; vb[k] has shape (count, s', s')."""
    flat = np.asarray(flat)
    S = sum(int(s) ** 2 for s in sizes)
    count = flat.size // S if S else 0
    assert count * S == flat.size
    per = flat.reshape(count, S)
    out, off = [], 0
    for s in sizes:
        B = per[:, off:off + s * s].reshape(count, s, s).transpose(0, 2, 1)  # column-major storage -> [class, row, col]
        out.append(embed(B) if np.iscomplexobj(flat) else B)
        off += s * s
    return out, count


def sparse_ref(flat, sizes, upper=True, tol=0.0, index_base=0):
    """dict(classptr int64[count + 1], blk / row / col int32, val float64, nnz): per class and block np.nonzero of the virtual
    block's mask, taken in column-major order (np.nonzero scans the TRANSPOSED block row-major)."""
    vb, count = virtual_blocks(flat, sizes)
    ci, bk, rr, cc, vv = [], [], [], [], []
    for k, M in enumerate(vb):
        with np.errstate(invalid="ignore"):
            mask = ~(np.abs(M) <= tol)
        if upper:
            mask &= np.triu(np.ones(M.shape[1:], dtype=bool))[None]
        i, c, r = np.nonzero(mask.transpose(0, 2, 1))  # sorted by class, then column, then row
        ci.append(i)
        bk.append(np.full(i.shape, k, dtype=np.int64))
        rr.append(r)
        cc.append(c)
        vv.append(M[i, r, c])
    ci, bk, rr, cc = (np.concatenate(a) if a else np.zeros(0, dtype=np.int64) for a in (ci, bk, rr, cc))
    vv = np.concatenate(vv) if vv else np.zeros(0)
    order = np.argsort(ci * len(sizes) + bk, kind="stable")  # classes in order, blocks in order inside a class, scan order kept
    ci, bk, rr, cc, vv = ci[order], bk[order], rr[order], cc[order], vv[order]
    classptr = np.zeros(count + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=count), out=classptr[1:])
    return {"classptr": classptr, "blk": (bk + index_base).astype(np.int32), "row": (rr + index_base).astype(np.int32),
            "col": (cc + index_base).astype(np.int32), "val": np.ascontiguousarray(vv, dtype=np.float64), "nnz": int(ci.size)}


def max_asym_ref(flat, sizes):
    """max over the virtual blocks and row < col of |M[row, col] - M[col, row]|; 0.0 for an empty window."""
    vb, count = virtual_blocks(flat, sizes)
    m = 0.0
    for M in vb:
        if M.size:
            m = max(m, float(np.abs(M - M.transpose(0, 2, 1)).max()))
    return m


def to_dense(sp, vsizes, count, index_base=0):
    """dense[i][k]: the entries put back into zero matrices of the virtual orders."""
    out = [[np.zeros((s, s)) for s in vsizes] for _ in range(count)]
    cls = np.repeat(np.arange(count), np.diff(sp["classptr"]))
    for e in range(sp["nnz"]):
        out[cls[e]][sp["blk"][e] - index_base][sp["row"][e] - index_base, sp["col"][e] - index_base] = sp["val"][e]
    return out
