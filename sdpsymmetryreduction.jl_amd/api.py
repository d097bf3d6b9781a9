"""Host-side mirror of the reference's interface for the Jordan-reduction path.

Same names, argument meaning and error behaviour as the Julia package
(``Partition``, ``dim``, ``refine``, ``fill``, ``randomize``, ``admissible_subspace``,
``diagonalize``, ``blockDiagonalize``); all computation happens in libsdpsr_hip.so
through the C ABI.  Arrays may be NumPy (host, copied by the library) or torch CUDA
tensors (device-resident, used in place).

Reference lines mirrored: src/partitions.jl:6-17,24-75,109-190; src/compat.jl:26-68;
src/diagonalize.jl:25-40,64-89; src/abstract_part.jl:7-16,107-110.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np

from . import _lib as L

RTOL_DEFAULT = math.sqrt(np.finfo(np.float64).eps)  # Base.rtoldefault(Float64)


class SdpsrError(RuntimeError):
    status = None


class InvalidDecompositionField(SdpsrError):
    """src/eigen_decomposition.jl:140-150"""


class NumericalInconsistency(SdpsrError):
    """src/eigen_decomposition.jl:152-161"""


class DimensionMismatch(SdpsrError):
    """src/diagonalize.jl:4-9"""


class LabelOverflow(SdpsrError):
    """InexactError of src/partitions.jl:63"""


class NotConverged(SdpsrError):
    pass


BAD_STATE = 10  # SDPSR_BAD_STATE

_EXC = {1: InvalidDecompositionField, 2: NumericalInconsistency, 3: DimensionMismatch,
        4: LabelOverflow, 9: NotConverged}


def _torch_label_dtype(bits):
    """torch dtype of a device-resident label array at ``bits`` bits per label (32: int32, the uint32 bit pattern)."""
    import torch
    return {8: torch.uint8, 16: getattr(torch, "uint16", torch.int16), 32: torch.int32}[int(bits)]


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)


class Context:
    """One device context = one HIP stream + workspace (sdpsr_create)."""

    def __init__(self, device=0, seed=0, square_mode=L.SQUARE_AUTO, channels=0, max_iters=0,
                 confirm_rounds=0, eig_driver=0, flags=0, round_mode="nearest", basis_image_kernel="auto",
                 refine_path="auto", label_bits=0, insert_wgs_per_cu=0, square_kernel=0, label_width=32,
                 psd_max_order=64):
        """``flags``: OR of ``_lib.FLAG_*``; ``round_mode``: "nearest" (default) or "trunc" (the
        reference's ``unsafe_round``, src/utils.jl:49-53); ``label_bits``: 0, or the width of the
        reference's label type ``T`` in ``Partition{T}`` to get ``LabelOverflow`` where it would throw
        inside the algorithms; ``label_width``: 32, 16 or 8 -- the element width of every label array this
        context passes to or receives from the library (``sdpsr_set_label_width``; ``Partition.matrix``
        then comes back as ``label_dtype``); ``psd_max_order``: 64 or 128 -- the largest block order ``psd_project``,
        ``BlockOperator.solve`` and ``reduce_and_solve`` take through this context (``sdpsr_set_psd_max_order``)."""
        self._lib = L.load_library()
        o = L.Opts()
        o.struct_size = C.sizeof(L.Opts)
        o.square_mode = int(square_mode)
        o.channels = int(channels)
        o.max_iters = int(max_iters)
        o.confirm_rounds = int(confirm_rounds)
        o.eig_driver = int(eig_driver)
        o.flags = int(flags)
        o.round_mode = {"nearest": L.ROUND_NEAREST, "trunc": L.ROUND_TRUNC}[round_mode] if isinstance(round_mode, str) else int(round_mode)
        o.basis_image_kernel = L.BASIS_IMAGE_KERNELS[basis_image_kernel] if isinstance(basis_image_kernel, str) else int(basis_image_kernel)
        o.refine_path = L.REFINE_PATHS[refine_path] if isinstance(refine_path, str) else int(refine_path)
        o.label_bits = int(label_bits)
        o.insert_wgs_per_cu = int(insert_wgs_per_cu)
        o.square_kernel = int(square_kernel)
        h = C.c_void_p()
        st = self._lib.sdpsr_create(int(device), C.c_uint64(seed & (2 ** 64 - 1)), C.byref(o), C.byref(h))
        if st != 0:
            raise SdpsrError(f"sdpsr_create failed: {L.STATUS.get(st, st)} (is a GPU visible?)")
        self._h = h
        self.device = device
        self._label_width = 32
        self._psd_max_order = 64
        try:
            if int(label_width) != 32:
                self.label_width = label_width
            if int(psd_max_order) != 64:
                self.psd_max_order = psd_max_order
        except Exception:
            self.close()
            raise

    @property
    def psd_max_order(self):
        """The largest block order of the PSD projection and the SDP solver through this context: 64 (default) or 128
        (``sdpsr_psd_max_order``)."""
        return self._psd_max_order

    @psd_max_order.setter
    def psd_max_order(self, order):
        if int(order) not in (64, 128):
            raise ValueError(f"psd_max_order is 64 or 128, got {order}")
        self.check(self._lib.sdpsr_set_psd_max_order(self._h, int(order)))
        self._psd_max_order = int(self._lib.sdpsr_psd_max_order(self._h))

    @property
    def label_width(self):
        """Bits of a label at this context's interface: 32 (default), 16 or 8 (``sdpsr_label_width``)."""
        return self._label_width

    @label_width.setter
    def label_width(self, bits):
        L.label_dtype(bits)  # ValueError for anything but 8 / 16 / 32
        self.check(self._lib.sdpsr_set_label_width(self._h, int(bits)))
        self._label_width = int(self._lib.sdpsr_label_width(self._h))

    @property
    def label_dtype(self):
        """NumPy dtype of the label arrays of this context (``np.uint8`` / ``np.uint16`` / ``np.uint32``)."""
        return L.label_dtype(self._label_width)

    def torch_label_dtype(self):
        """torch dtype of a device-resident label array of this context (32 bits: int32, the uint32 bit pattern)."""
        return _torch_label_dtype(self._label_width)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdpsr_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st == 0:
            return
        msg = self._lib.sdpsr_last_error(self._h).decode()
        exc = _EXC.get(st, SdpsrError)(msg or L.STATUS.get(st, str(st)))
        exc.status = st
        raise exc

    def set_seed(self, seed):
        self.check(self._lib.sdpsr_set_seed(self._h, C.c_uint64(seed & (2 ** 64 - 1))))

    def set_stream(self, stream_ptr):
        self.check(self._lib.sdpsr_set_stream(self._h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self.check(self._lib.sdpsr_synchronize(self._h))

    def dimension_trajectory(self):
        """dim(S) after the initial refinement and after every iteration of the last
        ``admissible_subspace`` on this context (what the reference logs under ``verbose``,
        src/partitions.jl:150,156,187-188)."""
        cnt = C.c_int32(0)
        self.check(self._lib.sdpsr_dimension_trajectory(self._h, None, 0, C.byref(cnt)))
        dims = np.zeros(max(cnt.value, 1), dtype=np.int64)
        self.check(self._lib.sdpsr_dimension_trajectory(self._h, dims.ctypes.data_as(C.c_void_p), cnt.value, C.byref(cnt)))
        return [int(x) for x in dims[:cnt.value]]

    def transfer_bytes(self):
        """(host -> device, device -> host) bytes this context has moved since its creation (``sdpsr_transfer_bytes``)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.check(self._lib.sdpsr_transfer_bytes(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def wait_for(self, *arrays):
        """Order ctx's stream behind torch's current stream when any argument is a CUDA tensor
        (it may have been produced by a kernel that is still running): sdpsr_wait_stream."""
        for a in arrays:
            if _is_torch(a) and a.is_cuda:
                import torch
                sp = torch.cuda.current_stream(a.device).cuda_stream
                self.check(self._lib.sdpsr_wait_stream(self._h, C.c_void_p(sp)))
                return


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def _ctx(ctx):
    return ctx if ctx is not None else default_context()


def _f(a, dtype):
    """Column-major flat host view of a matrix (the only order the reference scans)."""
    a = np.asarray(a, dtype=dtype)
    return np.ascontiguousarray(a.ravel(order="F"))


def _lab(matrix, ctx):
    """Column-major flat host labels at the context's width; a label that does not fit is the reference's InexactError."""
    a = np.asarray(matrix)
    dt = ctx.label_dtype
    if a.dtype != dt and a.size and (a.max() > np.iinfo(dt).max or a.min() < 0):
        exc = LabelOverflow(f"a label does not fit {dt.name} (the context's label_width is {ctx.label_width})")
        exc.status = 4
        raise exc
    return _f(a, dt)


class Partition:
    """``Partition`` (src/partitions.jl:6-17): ``matrix`` holds labels 0..nparts."""

    def __init__(self, nparts, matrix):
        self.nparts = int(nparts)
        self.matrix = matrix

    # --- constructors: Partition(M) float ctor (:24-35) / integer ctor (:37-42) ---
    @classmethod
    def from_matrix(cls, M, ctx=None):
        ctx = _ctx(ctx)
        M = np.asarray(M)
        shape = M.shape
        n = C.c_int64(0)
        out = np.empty(M.size, dtype=ctx.label_dtype)
        if np.issubdtype(M.dtype, np.floating):
            flat = _f(M, np.float64)
            ctx.check(ctx._lib.sdpsr_partition_from_f64(ctx._h, flat.size, _ptr(flat), _ptr(out), C.byref(n), L.MEM_HOST))
        else:
            if M.size and M.min() < 0:  # @assert 0 <= first(M_vals), src/partitions.jl:46
                raise ValueError("labels must be non-negative")
            if M.size and M.max() >= 2 ** 32:
                flat = _f(M, np.uint64)
                ctx.check(ctx._lib.sdpsr_partition_from_u64(ctx._h, flat.size, _ptr(flat), _ptr(out), C.byref(n), L.MEM_HOST))
            else:
                flat = _f(M, np.uint32)
                ctx.check(ctx._lib.sdpsr_partition_from_u32(ctx._h, flat.size, _ptr(flat), _ptr(out), C.byref(n), L.MEM_HOST))
        return cls(n.value, out.reshape(shape, order="F"))

    def __eq__(self, other):  # :16-17
        return self.nparts == other.nparts and np.array_equal(np.asarray(self.matrix), np.asarray(other.matrix))

    @property
    def shape(self):
        return tuple(self.matrix.shape)

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def __repr__(self):
        return f"Partition(dim={self.nparts}, size={self.shape})"


def dim(P):
    return P.nparts


def refine(P1, P2, ctx=None):
    """``refine!(P1, P2)`` (src/partitions.jl:62-66); P1 is updated and returned."""
    ctx = _ctx(ctx)
    assert P1.shape == P2.shape
    a = _lab(P1.matrix, ctx).copy()
    b = _lab(P2.matrix, ctx)
    d1 = C.c_int64(P1.nparts)
    ctx.check(ctx._lib.sdpsr_refine(ctx._h, a.size, _ptr(a), C.byref(d1), _ptr(b), P2.nparts, L.MEM_HOST))
    P1.matrix = a.reshape(P1.shape, order="F")
    P1.nparts = d1.value
    return P1


def partition_checksum(P, ctx=None):
    """128-bit checksum of the canonical label matrix: a probabilistic ``==`` of two partitions
    (src/partitions.jl:16-17) that avoids moving n^2 labels between GPUs.
    ``P`` is a Partition or a flat torch/NumPy array of column-major labels."""
    ctx = _ctx(ctx)
    if isinstance(P, Partition):
        lab, mem = _labels_arg(P, ctx)
    elif _is_torch(P):
        _check_torch_labels(P, ctx)
        lab, mem = P.contiguous().view(-1), (L.MEM_DEVICE if P.is_cuda else L.MEM_HOST)
    else:
        lab, mem = np.ascontiguousarray(_lab(np.asarray(P).ravel(), ctx)), L.MEM_HOST
    n_entries = lab.numel() if _is_torch(lab) else lab.size
    ctx.wait_for(lab)
    out = (C.c_uint64 * 2)()
    ctx.check(ctx._lib.sdpsr_partition_checksum(ctx._h, n_entries, _ptr(lab), C.cast(out, C.c_void_p), mem))
    return int(out[0]), int(out[1])


def relabel_keys(keys, ctx=None):
    """Canonical relabel (first-occurrence order, 0 stays 0) of a flat torch CUDA int64 tensor of
    arbitrary 64-bit keys, on the device: ``sdpsr_partition_from_u64``.  Returns (labels CUDA tensor -- int32 at the
    default label width --, nparts) -- the ``relabel`` callback of ``parallel.agree_partition`` on a GPU."""
    import torch
    ctx = _ctx(ctx)
    keys = keys.contiguous().view(-1)
    assert keys.is_cuda and keys.dtype == torch.int64
    out = torch.empty(keys.numel(), dtype=ctx.torch_label_dtype(), device=keys.device)
    n = C.c_int64(0)
    ctx.wait_for(keys)
    ctx.check(ctx._lib.sdpsr_partition_from_u64(ctx._h, keys.numel(), _ptr(keys), _ptr(out), C.byref(n), L.MEM_DEVICE))
    return out, n.value


def fill(P, values, ctx=None):
    """``fill!(M, P; values)`` (src/partitions.jl:68-75)."""
    ctx = _ctx(ctx)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if len(values) != P.nparts:  # @assert length(values) == dim(P), :69
        raise ValueError("length(values) != dim(P)")
    lab = _lab(P.matrix, ctx)
    out = np.empty(lab.size, dtype=np.float64)
    ctx.check(ctx._lib.sdpsr_fill(ctx._h, lab.size, _ptr(lab), _ptr(values), P.nparts, _ptr(out), L.MEM_HOST))
    return out.reshape(P.shape, order="F")


def randomize(P, ctx=None):
    """``randomize(P)`` (src/abstract_part.jl:97-110)."""
    ctx = _ctx(ctx)
    lab = _lab(P.matrix, ctx)
    out = np.empty(lab.size, dtype=np.float64)
    ctx.check(ctx._lib.sdpsr_randomize(ctx._h, lab.size, _ptr(lab), _ptr(out), L.MEM_HOST))
    return out.reshape(P.shape, order="F")


# ---------------------------------------------------------------------------
# admissible_subspace
# ---------------------------------------------------------------------------
def _dense(A):
    return np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)


def clamp_round_host(a, atol):
    """_clamp_round! (src/utils.jl:34-53), nearest rounding; host copy used only by the
    setup stage below (O(n^2), once)."""
    sig = math.floor(-math.log10(atol))
    scale = float(10 ** sig)
    x, e = np.frexp(a)
    out = np.ldexp(np.rint(scale * x) / scale, e)
    return np.where(np.abs(a) < atol, 0.0, out)


def admissible_setup(C_, A, b, atol=RTOL_DEFAULT):
    """Setup stage of ``admissible_subspace`` (src/partitions.jl:117-142), on the host:
    qr(A') -> orthonormal basis U of rowspace(A); C_L; min-norm x0 projected.
    Returns (n, CL, X0L, U) with CL/X0L flat column-major, U (n^2 x r) Fortran-ordered."""
    import scipy.linalg as sla
    c = np.asarray(C_.todense()).reshape(-1) if hasattr(C_, "todense") else np.asarray(C_, dtype=np.float64).reshape(-1)
    n = math.isqrt(len(c))
    if n * n != len(c):  # @assert n^2 == length(C), :118
        raise ValueError("length(C) is not a perfect square")
    Ad = np.asarray(_dense(A), dtype=np.float64)
    if Ad.shape[0] > 0:
        Q, R, _piv = sla.qr(Ad.T, mode="economic", pivoting=True)
        dg = np.abs(np.diag(R))
        r = int(np.sum(dg > 1e-12 * dg.max())) if dg.size and dg.max() > 0 else 0
        U = np.asfortranarray(Q[:, :r])
        # min-norm solution of A x = b (Krylov.craig, :137) from the factorisation at hand:
        # A[piv, :] = R' Q'  =>  x0 = Q_r y with R_rr' y = b[piv][:r]  (a LAPACK gelsd call on an
        # m x n^2 matrix with n^2 = 16.7M has been seen to crash inside the library)
        bb = np.asarray(b, dtype=np.float64)[_piv]
        y = sla.solve_triangular(R[:r, :r], bb[:r], trans="T", lower=False) if r else np.zeros(0)
        x0 = U @ y
    else:
        U = np.zeros((n * n, 0), order="F")
        x0 = np.zeros(n * n)

    def proj(v):
        return U @ (U.T @ v)

    def symm(v):
        M = v.reshape(n, n, order="F")
        return ((M + M.T) / 2).ravel(order="F")

    CL = symm(clamp_round_host(c - proj(c), atol))
    X0L = clamp_round_host(proj(symm(x0)), atol)
    CL, X0L = np.ascontiguousarray(CL), np.ascontiguousarray(X0L)
    m1, m2 = CL.reshape(n, n, order="F"), X0L.reshape(n, n, order="F")
    return Setup((n, CL, X0L, U), basis_is_symmetric(n, U), bool(np.array_equal(m1, m1.T) and np.array_equal(m2, m2.T)))


class Setup(tuple):
    """(n, CL, X0L, U) of ``admissible_setup`` plus what the host knows about symmetry:
    ``basis_symmetric`` (every column of U is a symmetric n x n matrix) and ``inputs_symmetric``
    (CL and X0L are exactly symmetric, as the reference's setup makes them).  ``hint`` is the bit
    mask for ``sdpsr_hint_symmetric_basis``."""

    def __new__(cls, items, basis_symmetric=False, inputs_symmetric=False, info=None):
        t = super().__new__(cls, items)
        t.info = info  # admissible_setup_csr: which orthogonalisation ran (_lib.SETUP_*); None for the host setup
        t.basis_symmetric = bool(basis_symmetric)
        t.inputs_symmetric = bool(inputs_symmetric)
        t.hint = (1 if basis_symmetric else 0) | (2 if inputs_symmetric else 0)
        return t


def basis_is_symmetric(n, U, tol=1e-12):
    """True if every column of U (n^2 x r), reshaped column-major to n x n, is symmetric."""
    U = np.asarray(U)
    for k in range(U.shape[1]):
        M = U[:, k].reshape(n, n, order="F")
        if not np.allclose(M, M.T, rtol=0.0, atol=tol):
            return False
    return True


def _admissible_subspace_device_setup(C_, A, b, atol, ctx, verbose):
    """Whole ``admissible_subspace`` through ``sdpsr_admissible_subspace_dense``: the setup stage
    (qr(A'), C_L, min-norm x0; src/partitions.jl:117-142) runs on the device as well."""
    c = np.asarray(C_.todense()).reshape(-1) if hasattr(C_, "todense") else np.asarray(C_, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.float64)
    n = math.isqrt(len(c))
    if n * n != len(c):
        raise ValueError("length(C) is not a perfect square")
    Ad = np.asfortranarray(_dense(A), dtype=np.float64)
    m = Ad.shape[0]
    bb = np.ascontiguousarray(b, dtype=np.float64)
    P = np.empty(n * n, dtype=ctx.label_dtype)
    d = C.c_int64(0)
    it = C.c_int32(0)
    ms = (C.c_double * L.T_COUNT)()
    ctx.check(ctx._lib.sdpsr_admissible_subspace_dense(ctx._h, n, m, _ptr(c), _ptr(Ad), _ptr(bb), float(atol), _ptr(P),
                                                       C.byref(d), C.byref(it), C.cast(ms, C.c_void_p), L.MEM_HOST))
    if verbose:
        print(f"[sdpsr] admissible subspace (device setup): dim {d.value} after {it.value} iterations, loop {ms[L.T_TOTAL]:.3f} ms")
    out = Partition(d.value, P.reshape(n, n, order="F"))
    out.iterations = it.value
    out.phase_ms = list(ms)
    out.dims = ctx.dimension_trajectory()
    return out


# ---------------------------------------------------------------------------
# setup from a sparse A (CSR), src/partitions.jl:117-142 on the device
# ---------------------------------------------------------------------------
def csr_arrays(A, len_, index_base=0):
    """Canonical 0-based CSR arrays (rowptr, colind, val) -- int64, int64, float64 -- of the m x ``len_`` constraint
    matrix ``A``: each row sorted by column, duplicates summed in input order, zeros dropped.  ``A`` is a SciPy sparse
    matrix in any format, a dense 2-D array, or a tuple ``(rowptr, colind, val)`` of CSR arrays with ``index_base`` 0 or 1
    (a Julia caller's ``sparse(A')`` colptr / rowval / nzval).  Malformed input raises ValueError."""
    len_ = int(len_)
    if isinstance(A, tuple):
        if len(A) != 3:
            raise ValueError("CSR input is a tuple (rowptr, colind, val)")
        if index_base not in (0, 1):
            raise ValueError("index_base must be 0 or 1")
        rowptr = np.asarray(A[0])
        colind = np.asarray(A[1])
        val = np.asarray(A[2], dtype=np.float64).ravel()
        if rowptr.ndim != 1 or rowptr.size < 1 or not np.issubdtype(rowptr.dtype, np.integer):
            raise ValueError("rowptr must be a non-empty integer vector")
        if colind.ndim != 1 or (colind.size and not np.issubdtype(colind.dtype, np.integer)):
            raise ValueError("colind must be an integer vector")
        rowptr = rowptr.astype(np.int64)
        colind = colind.astype(np.int64)
        if rowptr[0] != index_base:
            raise ValueError(f"rowptr[0] = {rowptr[0]} != index_base {index_base}")
        if np.any(np.diff(rowptr) < 0):
            raise ValueError("rowptr is not monotone")
        nnz = int(rowptr[-1] - index_base)
        if colind.size != nnz or val.size != nnz:
            raise ValueError(f"rowptr says {nnz} entries, colind has {colind.size}, val {val.size}")
        m = rowptr.size - 1
        rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptr))
        cols = colind - index_base
    elif hasattr(A, "tocsr"):  # SciPy: its compiled canonicalisation (O(nnz) per row sort, duplicates summed, zeros dropped)
        if A.ndim != 2 or A.shape[1] != len_:
            raise ValueError(f"A has shape {A.shape}, expected (m, {len_})")
        Ac = A.tocsr(copy=True).astype(np.float64)
        if not np.all(np.isfinite(Ac.data)):
            raise ValueError("non-finite value in A")
        Ac.sum_duplicates()
        Ac.eliminate_zeros()
        Ac.sort_indices()
        if not np.all(np.isfinite(Ac.data)):
            raise ValueError("duplicate entries sum to a non-finite value")
        return (Ac.indptr.astype(np.int64), Ac.indices.astype(np.int64), np.ascontiguousarray(Ac.data, dtype=np.float64))
    else:
        Ad = np.asarray(A, dtype=np.float64)
        if Ad.ndim != 2 or Ad.shape[1] != len_:
            raise ValueError(f"A has shape {Ad.shape}, expected (m, {len_})")
        m = Ad.shape[0]
        rows, cols = np.nonzero(Ad)
        rows, cols = rows.astype(np.int64), cols.astype(np.int64)
        val = Ad[rows, cols]
    if cols.size and (cols.min() < 0 or cols.max() >= len_):
        raise ValueError(f"column index outside [0, {len_})")
    if not np.all(np.isfinite(val)):
        raise ValueError("non-finite value in A")
    order = np.lexsort((cols, rows))  # stable: duplicates keep their input order
    rows, cols, val = rows[order], cols[order], val[order]
    if cols.size:
        first = np.ones(cols.size, dtype=bool)
        first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
        starts = np.flatnonzero(first)
        # left to right within a run, s = v0; s += v1; ... as the library's own pass adds them (np.add.reduceat adds the
        # tail of a run first, v0 + (v1 + v2): other bits): step k adds the k-th follower of every run that has one
        ends = np.append(starts[1:], cols.size)
        sums = val[starts].copy()
        k, live = 1, np.flatnonzero(ends - starts > 1)
        with np.errstate(over="ignore", invalid="ignore"):  # (a non-finite sum is reported below)
            while live.size:
                sums[live] += val[starts[live] + k]
                k += 1
                live = live[ends[live] - starts[live] > k]
        val = sums
        rows, cols = rows[starts], cols[starts]
        if not np.all(np.isfinite(val)):
            raise ValueError("duplicate entries sum to a non-finite value")
        keep = val != 0
        rows, cols, val = rows[keep], cols[keep], val[keep]
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=rowptr[1:])
    return rowptr, np.ascontiguousarray(cols, dtype=np.int64), np.ascontiguousarray(val, dtype=np.float64)


def _csr_inputs(C_, A, b, index_base):
    c = np.asarray(C_.todense()).reshape(-1) if hasattr(C_, "todense") else np.asarray(C_, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.float64)
    n = math.isqrt(len(c))
    if n * n != len(c):  # @assert n^2 == length(C), :118
        raise ValueError("length(C) is not a perfect square")
    rowptr, colind, val = csr_arrays(A, n * n, index_base)
    m = rowptr.size - 1
    bb = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
    if bb.size != m:
        raise ValueError(f"length(b) = {bb.size} != {m} rows of A")
    if not np.all(np.isfinite(bb)):
        raise ValueError("non-finite value in b")
    return n, c, m, rowptr, colind, val, bb


def _is_torch_sparse_csr(A):
    if not (hasattr(A, "layout") and hasattr(A, "crow_indices")):
        return False
    import torch
    return A.layout == torch.sparse_csr


def _raw_csr(A, len_, index_base):
    """The CSR arrays of ``A`` as they are -- no sorting, no summing, no dropping: that is the device's work
    (``SparseConstraints``).  Returns (rowptr, colind, val, index_base, on_device); ValueError for malformed shapes, dtypes
    and lengths."""
    len_ = int(len_)
    if index_base not in (0, 1):
        raise ValueError("index_base must be 0 or 1")
    if _is_torch_sparse_csr(A):
        if A.dim() != 2 or A.shape[1] != len_:
            raise ValueError(f"A has shape {tuple(A.shape)}, expected (m, {len_})")
        if not A.is_cuda:
            raise ValueError("a torch sparse_csr A must be a CUDA tensor (pass a SciPy matrix or NumPy arrays for host data)")
        A, index_base = (A.crow_indices(), A.col_indices(), A.values()), 0
    if isinstance(A, tuple):
        if len(A) != 3:
            raise ValueError("CSR input is a tuple (rowptr, colind, val)")
        if all(_is_torch(x) for x in A):
            import torch
            rowptr, colind, val = A
            if not all(x.is_cuda for x in A):
                raise ValueError("the three CSR tensors must be CUDA tensors")
            if rowptr.dim() != 1 or rowptr.numel() < 1 or rowptr.dtype.is_floating_point or rowptr.dtype == torch.bool:
                raise ValueError("rowptr must be a non-empty integer vector")
            if colind.dim() != 1 or colind.dtype.is_floating_point or colind.dtype == torch.bool:
                raise ValueError("colind must be an integer vector")
            if val.dim() != 1 or val.numel() != colind.numel():
                raise ValueError(f"colind has {colind.numel()} entries, val {val.numel()}")
            return (rowptr.to(torch.int64).contiguous(), colind.to(torch.int64).contiguous(), val.to(torch.float64).contiguous(),
                    index_base, True)
        if any(_is_torch(x) for x in A):
            raise ValueError("CSR input mixes torch tensors and host arrays")
        rowptr = np.asarray(A[0])
        colind = np.asarray(A[1])
        val = np.asarray(A[2], dtype=np.float64).ravel()
        if rowptr.ndim != 1 or rowptr.size < 1 or not np.issubdtype(rowptr.dtype, np.integer):
            raise ValueError("rowptr must be a non-empty integer vector")
        if colind.ndim != 1 or (colind.size and not np.issubdtype(colind.dtype, np.integer)):
            raise ValueError("colind must be an integer vector")
        if colind.size != val.size:
            raise ValueError(f"colind has {colind.size} entries, val {val.size}")
    elif hasattr(A, "tocsr"):
        if A.ndim != 2 or A.shape[1] != len_:
            raise ValueError(f"A has shape {A.shape}, expected (m, {len_})")
        Ac = A.tocsr()
        rowptr, colind, val, index_base = Ac.indptr, Ac.indices, Ac.data, 0
    else:
        Ad = np.asarray(A, dtype=np.float64)
        if Ad.ndim != 2 or Ad.shape[1] != len_:
            raise ValueError(f"A has shape {Ad.shape}, expected (m, {len_})")
        rows, cols = np.nonzero(Ad)
        val = Ad[rows, cols]
        rowptr = np.zeros(Ad.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=Ad.shape[0]), out=rowptr[1:])
        colind, index_base = cols, 0
    return (np.ascontiguousarray(rowptr, dtype=np.int64), np.ascontiguousarray(colind, dtype=np.int64),
            np.ascontiguousarray(val, dtype=np.float64), index_base, False)


class SparseConstraints:
    """The m x ``len_`` constraint matrix ``A`` in canonical CSR form, device-resident (``sdpsr_sparse_create``): validated,
    sorted, duplicates summed in input order and zeros dropped by a pass that runs on the device, ONCE; ``admissible_setup_csr``,
    ``admissible_subspace`` and ``reduce_constraints_csr`` take it in place of ``A`` and read it where it lies (setup stage of
    src/partitions.jl:117-142, ``A * PMat`` of README.md:57-60).

    ``A``: a SciPy sparse matrix (its ``tocsr()`` arrays travel raw), a tuple ``(rowptr, colind, val)`` of NumPy arrays with
    ``index_base`` 0 or 1, a torch ``sparse_csr`` CUDA tensor, a tuple of three CUDA tensors (read in place; integer dtypes
    other than int64 are converted), or a dense 2-D array.  Malformed input raises ValueError -- shapes, dtypes and lengths
    before any library call, the content with the library's message."""

    def __init__(self, A, len_, ctx=None, index_base=0):
        self._h = None
        rowptr, colind, val, base, on_dev = _raw_csr(A, len_, index_base)
        m = int(rowptr.shape[0]) - 1
        nnz = int(colind.shape[0])
        self.ctx = _ctx(ctx)
        if on_dev:
            self.ctx.wait_for(rowptr, colind, val)
        h = C.c_void_p()
        st = self.ctx._lib.sdpsr_sparse_create(self.ctx._h, int(len_), m, nnz, _ptr(rowptr), _ptr(colind) if nnz else None,
                                               _ptr(val) if nnz else None, int(base), L.MEM_DEVICE if on_dev else L.MEM_HOST, C.byref(h))
        if st == 5:  # SDPSR_BAD_ARGUMENT: what csr_arrays raises for the same input
            raise ValueError(self.ctx._lib.sdpsr_last_error(self.ctx._h).decode())
        self.ctx.check(st)
        self._h = h
        ln, mm, nz, sym = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        self.ctx.check(self.ctx._lib.sdpsr_sparse_info(self._h, C.byref(ln), C.byref(mm), C.byref(nz), C.byref(sym)))
        self.len, self.m, self.nnz, self.rows_symmetric = int(ln.value), int(mm.value), int(nz.value), bool(sym.value)

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.sdpsr_sparse_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def arrays(self, index_base=0, device=False):
        """The canonical arrays (rowptr, colind, val) as int64 / int64 / float64 with ``index_base`` (``sdpsr_sparse_export``):
        NumPy arrays, or torch CUDA tensors with ``device=True``.  They go into ``csr_arrays`` consumers as they are."""
        ctx = self.ctx
        if device:
            import torch
            dev = torch.device("cuda", ctx.device)
            rowptr = torch.empty(self.m + 1, dtype=torch.int64, device=dev)
            colind = torch.empty(self.nnz, dtype=torch.int64, device=dev)
            val = torch.empty(self.nnz, dtype=torch.float64, device=dev)
            ctx.wait_for(rowptr)
        else:
            rowptr = np.empty(self.m + 1, dtype=np.int64)
            colind = np.empty(self.nnz, dtype=np.int64)
            val = np.empty(self.nnz, dtype=np.float64)
        ctx.check(ctx._lib.sdpsr_sparse_export(ctx._h, self._h, int(index_base), _ptr(rowptr), _ptr(colind) if self.nnz else None,
                                               _ptr(val) if self.nnz else None, L.MEM_DEVICE if device else L.MEM_HOST))
        return rowptr, colind, val


def _sparse_inputs(C_, A, b, ctx):
    c = np.asarray(C_.todense()).reshape(-1) if hasattr(C_, "todense") else np.asarray(C_, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.float64)
    n = math.isqrt(len(c))
    if n * n != len(c):  # @assert n^2 == length(C), :118
        raise ValueError("length(C) is not a perfect square")
    if n * n != A.len:
        raise ValueError(f"A has {A.len} columns, expected {n * n}")
    bb = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
    if bb.size != A.m:
        raise ValueError(f"length(b) = {bb.size} != {A.m} rows of A")
    if not np.all(np.isfinite(bb)):
        raise ValueError("non-finite value in b")
    return n, c, bb, (A.ctx if ctx is None else ctx)


def _admissible_setup_sparse(C_, A, b, atol, ctx):
    import torch
    n, c, bb, ctx = _sparse_inputs(C_, A, b, ctx)
    m = A.m
    dev = torch.device("cuda", ctx.device)
    CL = torch.empty(n * n, dtype=torch.float64, device=dev)
    X0L = torch.empty(n * n, dtype=torch.float64, device=dev)
    Ubuf = torch.empty((m, n * n), dtype=torch.float64, device=dev)  # U = Ubuf.t(): column-major n^2 x m
    r = C.c_int64(0)
    hint = C.c_int(0)
    info = C.c_int32(0)
    ctx.wait_for(CL)
    ctx.check(ctx._lib.sdpsr_admissible_setup_sparse(ctx._h, n, A._h, _ptr(bb), _ptr(c), float(atol), _ptr(CL), _ptr(X0L),
                                                     _ptr(Ubuf) if m > 0 else None, C.byref(r), C.byref(hint), C.byref(info), L.MEM_DEVICE))
    U = Ubuf.t()[:, :r.value]
    return Setup((n, CL, X0L, U), bool(hint.value & 1), bool(hint.value & 2), info=int(info.value))


def _admissible_subspace_sparse(C_, A, b, atol, ctx, verbose):
    n, c, bb, ctx = _sparse_inputs(C_, A, b, ctx)
    P = np.empty(n * n, dtype=ctx.label_dtype)
    d = C.c_int64(0)
    it = C.c_int32(0)
    ms = (C.c_double * L.T_COUNT)()
    ctx.check(ctx._lib.sdpsr_admissible_subspace_sparse(ctx._h, n, A._h, _ptr(bb), _ptr(c), float(atol), _ptr(P), C.byref(d), C.byref(it),
                                                        C.cast(ms, C.c_void_p), L.MEM_HOST))
    if verbose:
        print(f"[sdpsr] admissible subspace (sparse handle): dim {d.value} after {it.value} iterations, loop {ms[L.T_TOTAL]:.3f} ms")
    out = Partition(d.value, P.reshape(n, n, order="F"))
    out.iterations = it.value
    out.phase_ms = list(ms)
    out.dims = ctx.dimension_trajectory()
    return out


def admissible_setup_csr(C_, A, b, atol=RTOL_DEFAULT, ctx=None, index_base=0):
    """Setup stage of ``admissible_subspace`` (src/partitions.jl:117-142) on the DEVICE from a sparse ``A``
    (``sdpsr_admissible_setup_csr``): A travels as CSR, C_L, X0_L and the orthonormal basis U stay in device memory.
    ``A``: anything ``csr_arrays`` takes.  Returns a ``Setup`` of torch CUDA tensors ``(n, CL, X0L, U)`` (U: n^2 x r,
    column-major) with ``.hint`` (the symmetry bits the library proved) and ``.info`` (``_lib.SETUP_*``: which
    orthogonalisation ran); it goes to ``admissible_subspace(setup=...)``, ``Problem(setup=...)`` and
    ``jordan_reduce_batch(setup=...)`` as it is.  A ``SparseConstraints`` for ``A`` is read where it lies
    (``sdpsr_admissible_setup_sparse``): no host pass, no upload of A."""
    if isinstance(A, SparseConstraints):
        return _admissible_setup_sparse(C_, A, b, atol, ctx)
    import torch
    n, c, m, rowptr, colind, val, bb = _csr_inputs(C_, A, b, index_base)  # (ValueError before any library call)
    ctx = _ctx(ctx)
    dev = torch.device("cuda", ctx.device)
    CL = torch.empty(n * n, dtype=torch.float64, device=dev)
    X0L = torch.empty(n * n, dtype=torch.float64, device=dev)
    Ubuf = torch.empty((m, n * n), dtype=torch.float64, device=dev)  # U = Ubuf.t(): column-major n^2 x m
    r = C.c_int64(0)
    hint = C.c_int(0)
    info = C.c_int32(0)
    ctx.wait_for(CL)
    ctx.check(ctx._lib.sdpsr_admissible_setup_csr(ctx._h, n, m, _ptr(rowptr), _ptr(colind), _ptr(val), 0, _ptr(bb), _ptr(c), float(atol),
                                                  _ptr(CL), _ptr(X0L), _ptr(Ubuf) if m > 0 else None, C.byref(r), C.byref(hint),
                                                  C.byref(info), L.MEM_DEVICE))
    U = Ubuf.t()[:, :r.value]
    return Setup((n, CL, X0L, U), bool(hint.value & 1), bool(hint.value & 2), info=int(info.value))


def _admissible_subspace_csr(C_, A, b, atol, ctx, verbose):
    """Whole ``admissible_subspace`` through ``sdpsr_admissible_subspace_csr``: A uploaded as CSR, the setup stage on
    the device, then the loop."""
    n, c, m, rowptr, colind, val, bb = _csr_inputs(C_, A, b, 0)
    ctx = _ctx(ctx)
    P = np.empty(n * n, dtype=ctx.label_dtype)
    d = C.c_int64(0)
    it = C.c_int32(0)
    ms = (C.c_double * L.T_COUNT)()
    ctx.check(ctx._lib.sdpsr_admissible_subspace_csr(ctx._h, n, m, _ptr(rowptr), _ptr(colind), _ptr(val), 0, _ptr(bb), _ptr(c), float(atol),
                                                     _ptr(P), C.byref(d), C.byref(it), C.cast(ms, C.c_void_p), L.MEM_HOST))
    if verbose:
        print(f"[sdpsr] admissible subspace (CSR setup): dim {d.value} after {it.value} iterations, loop {ms[L.T_TOTAL]:.3f} ms")
    out = Partition(d.value, P.reshape(n, n, order="F"))
    out.iterations = it.value
    out.phase_ms = list(ms)
    out.dims = ctx.dimension_trajectory()
    return out


def admissible_subspace(C_, A, b, atol=RTOL_DEFAULT, ctx=None, verbose=False, setup=None,
                        return_info=False, host_setup=False, csr_setup=False):
    """``admissible_subspace(C, A, b; verbose, atol)`` (src/partitions.jl:77-190).

    By default the setup stage runs on the device too (dense copy of ``A``, at most 4 GiB);
    ``host_setup=True`` (or a precomputed ``setup``) uses the NumPy/SciPy setup, which is also the
    path for very large sparse ``A``.  ``csr_setup=True`` (opt-in) sends ``A`` as CSR and runs the setup
    stage on the device from it (``sdpsr_admissible_subspace_csr``): no dense copy of ``A`` anywhere.  A
    ``SparseConstraints`` for ``A`` always takes its own entry (``sdpsr_admissible_subspace_sparse``)."""
    if setup is None and isinstance(A, SparseConstraints):
        return _admissible_subspace_sparse(C_, A, b, atol, ctx, verbose)
    if setup is None and csr_setup and not host_setup:
        return _admissible_subspace_csr(C_, A, b, atol, ctx, verbose)
    ctx = _ctx(ctx)
    if setup is None and not host_setup and A is not None:
        m_rows = A.shape[0]
        if m_rows * int(np.prod(np.shape(C_))) * 8 <= (4 << 30):
            return _admissible_subspace_device_setup(C_, A, b, atol, ctx, verbose)
    if setup is None:
        setup = admissible_setup(C_, A, b, atol)
    n, CL, X0L, U = setup
    if getattr(setup, "hint", 0):
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, int(setup.hint))  # applies to the call below only
    on_dev = _is_torch(CL)
    r = U.shape[1]
    if on_dev:
        import torch
        P = torch.empty(n * n, dtype=ctx.torch_label_dtype(), device=CL.device)  # (32 bits: the uint32 bit pattern)
    else:
        U = np.asfortranarray(U, dtype=np.float64)
        P = np.empty(n * n, dtype=ctx.label_dtype)
    d = C.c_int64(0)
    it = C.c_int32(0)
    ms = (C.c_double * L.T_COUNT)()
    ctx.wait_for(CL, X0L, U)
    st = ctx._lib.sdpsr_admissible_subspace(
        ctx._h, n, _ptr(CL), _ptr(X0L), _ptr(U) if r > 0 else None, r, float(atol), _ptr(P),
        C.byref(d), C.byref(it), C.cast(ms, C.c_void_p), L.MEM_DEVICE if on_dev else L.MEM_HOST)
    ctx.check(st)
    out_dims = ctx.dimension_trajectory()
    if verbose:
        print(f"[sdpsr] Starting the reduction. Dimensions: maximal = {(n * n + n) // 2}, initial = {out_dims[0] if out_dims else '?'}")
        for k, dk in enumerate(out_dims[:-1]):
            print(f"[sdpsr] Iteration {k + 1}, Current dimension: {dk}")
        print(f"[sdpsr] admissible subspace: dim {d.value} after {it.value} iterations, "
              f"{ms[L.T_TOTAL]:.3f} ms (project {ms[L.T_PROJECT]:.3f}, square {ms[L.T_SQUARE]:.3f}, "
              f"refine {ms[L.T_REFINE]:.3f})")
    mat = P.view(n, n).t() if on_dev else P.reshape(n, n, order="F")
    out = Partition(d.value, mat)
    out.iterations = it.value
    out.phase_ms = list(ms)
    out.dims = out_dims
    return out


class Problem:
    """The loop's inputs (C_L, X0_L, U of ``admissible_setup``) made device-resident ONCE (``sdpsr_problem_create``); any
    number of ``reduce`` / ``reduce_batch`` calls then read them there.  The reference's seam hands host arrays to
    ``admissible_subspace`` on every call (src/partitions.jl:109-116); restarting the randomized reduction of one problem
    ("try again", src/eigen_decomposition.jl:264-270) through it pays the upload -- 3 x 134 MB at N = 4096 -- every time."""

    def __init__(self, C_=None, A=None, b=None, atol=RTOL_DEFAULT, ctx=None, setup=None):
        self.ctx = _ctx(ctx)
        setup = setup if setup is not None else admissible_setup(C_, A, b, atol)
        self.n, CL, X0L, U = setup
        self.r = U.shape[1]
        self.atol = atol
        if _is_torch(CL):  # a device setup (admissible_setup_csr): read in place, copied device to device
            ln = self.n * self.n
            CL, X0L = CL.contiguous(), X0L.contiguous()
            Uf = (U if U.stride() == (1, ln) else U.t().contiguous().t()) if self.r else None
            mem = L.MEM_DEVICE
            self.ctx.wait_for(CL, X0L, Uf if self.r else CL)
        else:
            Uf = np.asfortranarray(U) if self.r else None
            mem = L.MEM_HOST
        h = C.c_void_p()
        self.ctx.check(self.ctx._lib.sdpsr_problem_create(self.ctx._h, self.n, _ptr(CL), _ptr(X0L), _ptr(Uf) if self.r else None, self.r,
                                                          int(getattr(setup, "hint", 0)), mem, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.sdpsr_problem_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reduce(self, seed=None, epsilon=RTOL_DEFAULT, atol=None):
        """One reduction (``admissible_subspace`` + ``blockDiagonalize``): the dict of a one-restart batch; raises the
        reference's exception for a status that is not 0."""
        res = self.reduce_batch(1, seeds=None if seed is None else [seed], epsilon=epsilon, atol=atol)[0]
        if res["status"]:
            self.ctx.check(res["status"])
        return res

    def reduce_batch(self, restarts=2, seeds=None, epsilon=RTOL_DEFAULT, atol=None):
        """``restarts`` independent random restarts in one call (``sdpsr_problem_reduce_batch``); a list of dicts as
        ``jordan_reduce_batch`` returns them."""
        ctx, lib, n = self.ctx, self.ctx._lib, self.n
        R = int(restarts)
        atol = self.atol if atol is None else atol
        if seeds is None:  # explicit seeds: the sizes call and the images call must run the same restarts
            seeds = [int(x) for x in np.random.SeedSequence().generate_state(R, dtype=np.uint64)]
        if len(seeds) != R:
            raise ValueError(f"{len(seeds)} seeds for {R} restarts")
        sd = (C.c_uint64 * R)(*[int(x) & (2 ** 64 - 1) for x in seeds])
        label_dt = L.label_dtype(getattr(ctx, "label_width", 32))  # (a context-like object without a width: the ABI's default)

        def call(blk_arrays):
            Ps = [np.zeros(n * n, dtype=label_dt) for _ in range(R)]
            pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
            dd, it, nb = (C.c_int64 * R)(), (C.c_int32 * R)(), (C.c_int32 * R)()
            ssq, ss = (C.c_int64 * R)(), (C.c_int64 * R)()
            st = (C.c_int32 * R)(*([-1] * R))  # a sentinel no status code has
            pb = caps = None
            if blk_arrays is not None:
                pb = (C.c_void_p * R)(*[a.ctypes.data for a in blk_arrays])
                caps = (C.c_int64 * R)(*[a.size for a in blk_arrays])
            rc = lib.sdpsr_problem_reduce_batch(ctx._h, self._h, R, C.cast(sd, C.c_void_p), atol, epsilon, C.cast(pP, C.c_void_p), dd, it, nb, ssq, ss,
                                                C.cast(pb, C.c_void_p) if pb is not None else None, caps, st, L.MEM_HOST)
            # the call's own status counts unless some restart reports one: a failure before the restarts start (bad
            # arguments, memory) must not read as R clean restarts of dimension 0.  The library presets every status to
            # BAD_STATE before anything can fail; -1 is this binding's own sentinel.
            if rc != 0 and (all(x in (-1, BAD_STATE) for x in st) or all(x in (0, -1) for x in st)):
                ctx.check(rc)
            return Ps, dd, it, nb, ssq, ss, st

        Ps, dd, it, nb, ssq, ss, st = call(None)  # sizes first, then the images into buffers of the right size
        bl = [np.zeros(max(1, dd[i] * ssq[i])) for i in range(R)]
        Ps, dd, it, nb, ssq, ss, st = call(bl)
        out = []
        for i in range(R):
            status, blks = int(st[i]), None
            if status == 0:
                if dd[i] * ssq[i] <= bl[i].size:
                    blks = bl[i][:dd[i] * ssq[i]].reshape(dd[i], ssq[i])
                else:  # the images pass ran another reduction than the sizes pass: its images were never written
                    status = BAD_STATE
            out.append({"status": status, "P": Partition(int(dd[i]), Ps[i].reshape(n, n, order="F")), "iterations": int(it[i]),
                        "nblocks": int(nb[i]), "sum_sq": int(ssq[i]), "sum_s": int(ss[i]), "blks": blks})
        return out


def jordan_reduce_batch(C_, A, b, restarts=2, seeds=None, atol=RTOL_DEFAULT, epsilon=RTOL_DEFAULT, ctx=None, setup=None):
    """``restarts`` independent random restarts of ``admissible_subspace`` + ``blockDiagonalize`` of one problem in ONE
    call on one host thread: restart i with its own random streams, HIP stream and workspace; while one restart's host
    side waits for a verdict the others' work is submitted.  The reference's answer to the randomized failures of
    ``blockDiagonalize`` is "try again" (src/eigen_decomposition.jl:264-270, src/diagonalize.jl:4-9): here the tries run
    side by side and the caller takes the first whose status is 0.  The problem is uploaded once (``Problem``) and both
    passes -- sizes, then images -- read it on the device; ``seeds=None`` draws explicit seeds, so that the two passes run
    the same restarts.  Returns a list of dicts: status, P (Partition), iterations, nblocks, sum_sq, sum_s, blks
    (d x sum s_k^2 array, class-major; None for a restart whose status is not 0)."""
    with Problem(C_, A, b, atol=atol, ctx=ctx, setup=setup) as prob:
        return prob.reduce_batch(restarts, seeds=seeds, epsilon=epsilon)


def reduce_constraints(P, A, ctx=None):
    """``A * PMat`` with ``PMat = hcat([vec(P.matrix .== i) for i = 1:dim(P)]...)``
    (README.md:57-60, test/sd_problems.jl:32-37); ``A`` dense m x n^2 (or a vector: C' * PMat).  A sparse ``A`` is
    densified here, and the accumulators must fit the LDS ((dim(P) + 1) * min(m, 64) doubles in 60 KiB):
    ``reduce_constraints_csr`` takes a sparse ``A`` as it is, for any dim(P)."""
    ctx = _ctx(ctx)
    A = np.asarray(_dense(A), dtype=np.float64)
    vec = A.ndim == 1
    A2 = A.reshape(1, -1) if vec else A
    m, ln = A2.shape
    lab = _lab(P.matrix, ctx)
    assert ln == lab.size
    Af = np.asfortranarray(A2)
    out = np.zeros((m, P.nparts), order="F")
    ctx.check(ctx._lib.sdpsr_reduce_constraints(ctx._h, ln, _ptr(lab), P.nparts, m, _ptr(Af), _ptr(out), L.MEM_HOST))
    return out[0] if vec else out


def _reduce_constraints_sparse(P, A, ln, ctx, keep_on_device=False):
    """keep_on_device (device labels only): the flat m * d device buffer the entry filled comes back as it is."""
    if ln != A.len:
        raise ValueError(f"A has {A.len} columns, P has {ln} entries")
    m, d = A.m, int(P.nparts)
    if not 1 <= d <= ln:
        raise ValueError(f"dim(P) = {d} outside [1, {ln}]")
    ctx = A.ctx if ctx is None else ctx
    lab, mem = _labels_arg(P, ctx)
    if mem == L.MEM_DEVICE:
        import torch
        t_out = torch.empty(m * d, dtype=torch.float64, device=lab.device)
        ctx.wait_for(lab, t_out)
        ctx.check(ctx._lib.sdpsr_reduce_constraints_sparse(ctx._h, A._h, _ptr(lab), d, _ptr(t_out), mem))
        if keep_on_device:
            return t_out
        return t_out.cpu().numpy().reshape(m, d, order="F")
    out = np.zeros((m, d), order="F")
    ctx.check(ctx._lib.sdpsr_reduce_constraints_sparse(ctx._h, A._h, _ptr(lab), d, _ptr(out), mem))
    return out


def reduce_constraints_csr(P, A, ctx=None, index_base=0):
    """``A * PMat`` (README.md:57-60, test/sd_problems.jl:32-37,113-118) from a sparse ``A``, for any dim(P)
    (``sdpsr_reduce_constraints_csr``): A travels as CSR and is never densified.  ``A``: anything ``csr_arrays`` takes
    -- SciPy sparse, dense 2-D, or ``(rowptr, colind, val)`` with ``index_base`` -- with n^2 columns; returns an
    m x dim(P) NumPy array.  A 1-D array or a SciPy-sparse vector (n^2 x 1, or 1-D) means ``C' * PMat``: a vector of
    length dim(P) comes back.  Malformed input raises ValueError before any library call.  Equal inputs give equal bits.
    A ``SparseConstraints`` for ``A`` is read where it lies (``sdpsr_reduce_constraints_sparse``)."""
    ln = int(P.shape[0]) * int(P.shape[1])
    vec = False
    if isinstance(A, SparseConstraints):
        return _reduce_constraints_sparse(P, A, ln, ctx)
    if not isinstance(A, tuple):
        if hasattr(A, "tocsr"):
            if A.ndim == 1:
                vec, A = True, A.reshape(1, -1)
            elif A.shape[1] == 1 and ln != 1:
                vec, A = True, A.T
        else:
            A = np.asarray(A, dtype=np.float64)
            if A.ndim == 1:
                vec, A = True, A.reshape(1, -1)
    rowptr, colind, val = csr_arrays(A, ln, index_base)  # (ValueError before any library call)
    m, d = rowptr.size - 1, int(P.nparts)
    if not 1 <= d <= ln:
        raise ValueError(f"dim(P) = {d} outside [1, {ln}]")
    ctx = _ctx(ctx)
    lab, mem = _labels_arg(P, ctx)
    if mem == L.MEM_DEVICE:
        import torch
        t_out = torch.empty(m * d, dtype=torch.float64, device=lab.device)
        ctx.wait_for(lab, t_out)
        ctx.check(ctx._lib.sdpsr_reduce_constraints_csr(ctx._h, ln, _ptr(lab), d, m, _ptr(rowptr), _ptr(colind), _ptr(val), 0,
                                                        _ptr(t_out), mem))
        out = t_out.cpu().numpy().reshape(m, d, order="F")
    else:
        out = np.zeros((m, d), order="F")
        ctx.check(ctx._lib.sdpsr_reduce_constraints_csr(ctx._h, ln, _ptr(lab), d, m, _ptr(rowptr), _ptr(colind), _ptr(val), 0,
                                                        _ptr(out), mem))
    return out[0] if vec else out


def compress_constraints(newA, b=None, rtol=0.0, droptol=1e-8, ctx=None, return_info=False, m=None):
    """The independent part of the reduced constraints ``newA * x = b``: an orthonormal basis of the row space of
    ``[newA b]`` (docs/src/examples/ReduceAndSolveJuMP.jl:44-50: ``svd(Matrix(hcat(A * PMat, b))').U[:, 1:rank]'``, then
    ``droptol!``; ``sdpsr_compress_constraints``).  Returns ``(newA2, newB2)`` of shapes r x d and r -- ``newA2`` alone when
    ``b`` is None -- with r the number of singular values above ``rtol * sigma_1`` (``rtol = 0``: Julia's ``rank`` default
    ``min(size) * eps``); row k belongs to the k-th largest singular value, is normalised, has its first entry of largest
    magnitude positive, and its entries with ``|v| <= droptol`` are exactly 0.  ``return_info=True`` adds a dict with ``rank``,
    ``sv`` (all m singular values, descending), ``nnz`` and ``passes``.

    ``newA``: an m x d NumPy array, or a torch CUDA tensor -- m x d with column-major strides, or the flat ``m * d`` buffer the
    sparse assembly fills (then ``m`` names the row count).  Device input is read where it lies and the result comes back as
    device tensors; ``b`` is host data either way."""
    ctx = _ctx(ctx)
    lib = ctx._lib
    bh = None if b is None else np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
    if _is_torch(newA):
        import torch
        if not newA.is_cuda or newA.dtype != torch.float64:
            raise TypeError("a torch newA is a float64 CUDA tensor")
        if newA.dim() == 1:
            if m is None:
                if bh is None:
                    raise ValueError("a flat newA needs m (or b, whose length is m)")
                m = bh.size
            mm = int(m)
            if mm < 0 or (mm == 0 and newA.numel()) or (mm and newA.numel() % mm):
                raise ValueError(f"a flat newA of {newA.numel()} entries has no {mm} rows")
            d = newA.numel() // mm if mm else 0
            flat = newA.contiguous()
        else:
            if newA.dim() != 2:
                raise ValueError("newA is a matrix")
            mm, d = int(newA.shape[0]), int(newA.shape[1])
            flat = newA.t().contiguous().view(-1)  # (no copy when newA has column-major strides)
        mem = L.MEM_DEVICE
    else:
        A2 = np.asfortranarray(np.asarray(_dense(newA), dtype=np.float64))
        if A2.ndim != 2:
            raise ValueError("newA is a matrix")
        mm, d = A2.shape
        flat, mem = A2, L.MEM_HOST
    if bh is not None and bh.size != mm:
        raise ValueError(f"b has {bh.size} entries, newA has {mm} rows")
    ncols = d + (bh is not None)
    if mem == L.MEM_DEVICE:
        import torch
        out = torch.empty(mm * ncols, dtype=torch.float64, device=flat.device)
        ctx.wait_for(flat, out)
    else:
        out = np.zeros((mm, ncols), order="F")
    rank, nnz, passes = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    sv = np.zeros(mm)
    ctx.check(lib.sdpsr_compress_constraints(ctx._h, mm, d, _ptr(flat) if mm * d else None, _ptr(bh), float(rtol), float(droptol),
                                             _ptr(out) if mm * ncols else None, C.byref(rank), _ptr(sv), C.byref(nnz),
                                             C.byref(passes), mem))
    r = int(rank.value)
    if mem == L.MEM_DEVICE:
        M2 = out.view(ncols, mm).t()[:r]  # (the r x ncols view of the column-major buffer)
    else:
        M2 = out[:r]
    res = M2 if bh is None else (M2[:, :d], M2[:, d])
    if not return_info:
        return res
    info = {"rank": r, "sv": sv, "nnz": int(nnz.value), "passes": int(passes.value)}
    return (res, info) if bh is None else res + (info,)


def reduced_sdp(P, A, b, C_, compress=True, rtol=0.0, droptol=1e-8, ctx=None):
    """The whole hand-over of docs/src/examples/ReduceAndSolveJuMP.jl:42-51 in one call: ``(newA, newB, newC)`` with
    ``newC = C' * PMat`` and ``[newA newB]`` the independent rows of ``[A * PMat  b]`` (``compress_constraints``;
    ``compress=False``: ``A * PMat`` and ``b`` as they are).  ``A`` decides the assembly: a ``SparseConstraints`` is read
    where it lies, SciPy-sparse input or a ``(rowptr, colind, val)`` triple goes through ``reduce_constraints_csr``, a dense
    array through ``reduce_constraints``; ``newC`` takes the same route.  With a ``SparseConstraints`` and device-resident
    labels ``A * PMat`` stays on the device between the assembly and the compression, and ``newA`` / ``newB`` come back as
    device tensors."""
    ln = int(P.shape[0]) * int(P.shape[1])
    bh = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
    c = np.asarray(_dense(C_), dtype=np.float64).reshape(-1, order="F")
    if isinstance(A, SparseConstraints):
        cx = A.ctx if ctx is None else ctx
        with SparseConstraints(c.reshape(1, -1), ln, ctx=cx) as Cs:
            newC = _reduce_constraints_sparse(P, Cs, ln, cx)[0]
        on_device = _is_torch(P.matrix)
        newA = _reduce_constraints_sparse(P, A, ln, cx, keep_on_device=on_device)
        m = A.m
    elif isinstance(A, tuple) or hasattr(A, "tocsr"):
        cx = _ctx(ctx)
        newA, newC = reduce_constraints_csr(P, A, ctx=cx), reduce_constraints_csr(P, c, ctx=cx)
        m = newA.shape[0]
    else:
        cx = _ctx(ctx)
        newA, newC = reduce_constraints(P, A, ctx=cx), reduce_constraints(P, c, ctx=cx)
        m = newA.shape[0]
    if bh.size != m:
        raise ValueError(f"b has {bh.size} entries, A has {m} rows")
    if not compress:
        if _is_torch(newA):
            newA = newA.view(-1, m).t()
        return newA, bh, newC
    newA2, newB2 = compress_constraints(newA, bh, rtol=rtol, droptol=droptol, ctx=cx, m=m)
    return newA2, newB2, newC


def desymmetrize(P, ctx=None):
    """``desymmetrize(P)`` (src/partitions.jl:197-223); returns a new Partition."""
    ctx = _ctx(ctx)
    n = P.shape[0]
    lab = _lab(P.matrix, ctx).copy()
    d = C.c_int64(P.nparts)
    it = C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_desymmetrize(ctx._h, n, _ptr(lab), C.byref(d), C.byref(it), L.MEM_HOST))
    out = Partition(d.value, lab.reshape(P.shape, order="F"))
    out.iterations = it.value
    return out


unSymmetrize = desymmetrize  # src/compat.jl:70


# ---------------------------------------------------------------------------
# blockDiagonalize
# ---------------------------------------------------------------------------
BlockDiagonalization = namedtuple("BlockDiagonalization", ["blkSizes", "blks", "Q_hat", "phase_ms"])
ComplexBlockDiagonalization = namedtuple("ComplexBlockDiagonalization", ["blkSizes", "blks", "Q_hat", "partition"])


def _check_torch_labels(t, ctx):
    if t.element_size() * 8 != ctx.label_width or t.dtype.is_floating_point:
        raise TypeError(f"a torch label array of this context has {ctx.label_width}-bit integer elements "
                        f"({ctx.torch_label_dtype()}), not {t.dtype}: convert with labels_convert")


def _labels_arg(P, ctx=None):
    ctx = _ctx(ctx)
    m = P.matrix
    if _is_torch(m):
        _check_torch_labels(m, ctx)
        # stored as the transposed view of a flat column-major buffer (see admissible_subspace)
        flat = m.t().contiguous().view(-1)
        return flat, L.MEM_DEVICE
    return _lab(m, ctx), L.MEM_HOST


def labels_convert(a, bits, ctx=None):
    """Element-wise conversion of a label array to ``bits`` = 8, 16 or 32 bits per label on the device
    (``sdpsr_labels_convert``): a NumPy array of uint8 / uint16 / uint32 (copied by the library) or a torch CUDA tensor
    with 1-, 2- or 4-byte integer elements (converted where it lies).  Returns a new array of the same kind and shape;
    raises ``LabelOverflow`` when a value does not fit.  Independent of the context's own ``label_width``."""
    ctx = _ctx(ctx)
    out_dt = L.label_dtype(bits)
    if _is_torch(a):
        import torch
        if a.dtype.is_floating_point or a.element_size() not in (1, 2, 4) or not a.is_cuda:
            raise TypeError("labels_convert takes a CUDA tensor of 1-, 2- or 4-byte integers")
        src = a.contiguous()
        out = torch.empty(src.shape, dtype=_torch_label_dtype(bits), device=src.device)
        ctx.wait_for(src, out)
        ctx.check(ctx._lib.sdpsr_labels_convert(ctx._h, src.numel(), _ptr(src), src.element_size() * 8, _ptr(out), int(bits), L.MEM_DEVICE))
        return out
    src = np.ascontiguousarray(a)
    if src.dtype not in L.LABEL_DTYPES.values():
        raise TypeError("labels_convert takes uint8, uint16 or uint32 labels")
    out = np.empty(src.shape, dtype=out_dt)
    ctx.check(ctx._lib.sdpsr_labels_convert(ctx._h, src.size, _ptr(src), src.dtype.itemsize * 8, _ptr(out), int(bits), L.MEM_HOST))
    return out


def blockDiagonalize(P, verbose=False, epsilon=RTOL_DEFAULT, complex=False, ctx=None, retries=0):
    """``blockDiagonalize(P, verbose; epsilon, complex)`` (src/compat.jl:26-68), real path.

    ``retries`` > 0 re-runs the randomized decomposition with fresh generic elements when it ends
    in ``NumericalInconsistency`` / ``DimensionMismatch`` -- what the reference's error texts ask
    the caller to do ("try again"); the default 0 is the reference's behaviour."""
    ctx = _ctx(ctx)
    if complex:
        return _block_diagonalize_complex(P, verbose, epsilon, ctx, retries)
    for attempt in range(int(retries)):
        try:
            return blockDiagonalize(P, verbose=verbose, epsilon=epsilon, ctx=ctx, retries=0)
        except (NumericalInconsistency, DimensionMismatch) as e:
            if verbose:
                print(f"[sdpsr] blockDiagonalize attempt {attempt + 1} failed ({type(e).__name__}); retrying")
    n = P.shape[0]
    lab, mem = _labels_arg(P, ctx)
    ctx.wait_for(lab)
    nb = C.c_int32(0)
    ssq = C.c_int64(0)
    ss = C.c_int64(0)
    ms1 = (C.c_double * L.T_COUNT)()
    ctx.check(ctx._lib.sdpsr_block_diagonalize(ctx._h, n, _ptr(lab), P.nparts, float(epsilon), C.byref(nb),
                                               C.byref(ssq), C.byref(ss), C.cast(ms1, C.c_void_p), mem))
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, _ptr(sizes)))
    blks = np.empty(P.nparts * ssq.value, dtype=np.float64)
    qh = np.empty(n * ss.value, dtype=np.float64)
    ms2 = (C.c_double * L.T_COUNT)()
    ctx.check(ctx._lib.sdpsr_block_images(ctx._h, _ptr(blks), _ptr(qh), C.cast(ms2, C.c_void_p), L.MEM_HOST))
    out = []
    blks = blks.reshape(P.nparts, ssq.value) if ssq.value else blks.reshape(P.nparts, 0)
    for i in range(P.nparts):
        row, off = [], 0
        for s in sizes:
            row.append(blks[i, off:off + s * s].reshape(s, s, order="F"))
            off += s * s
        out.append(row)
    Q, off = [], 0
    qh = qh.reshape(n, ss.value, order="F")
    for s in sizes:
        Q.append(qh[:, off:off + s])
        off += s
    ms = [a + b for a, b in zip(ms1, ms2)]
    if verbose:
        print(f"[sdpsr] blockDiagonalize: blocks {list(sizes)}; eigen {ms[L.T_EIGEN]:.3f} ms, iso {ms[L.T_ISO]:.3f}, "
              f"irreducible {ms[L.T_IRRED]:.3f}, image {ms[L.T_IMAGE]:.3f}")
    return BlockDiagonalization([int(s) for s in sizes], out, Q, ms)


def class_window(d, parts, index):
    """``(first, count)``: window ``index`` (0-based) of ``parts`` contiguous windows that tile the classes ``1..d`` in
    order, their sizes differing by at most one (the larger ones first); ``count == 0`` -- with ``first`` where the window
    would start -- once ``parts > d`` leaves nothing for this index.  Pure arithmetic: every rank computes its own."""
    d, parts, index = int(d), int(parts), int(index)
    if d < 0 or parts < 1 or not 0 <= index < parts:
        raise ValueError(f"class_window(d={d}, parts={parts}, index={index}): need d >= 0, parts >= 1, 0 <= index < parts")
    q, r = divmod(d, parts)
    return 1 + index * q + min(index, r), q + (1 if index < r else 0)


def _is_complex(x):
    """A NumPy or torch array of complex64 / complex128 elements."""
    if _is_torch(x):
        return x.is_complex()
    return np.iscomplexobj(x)


def _q_hat_arg(Q_hat, n):
    """(matrix, sizes) from a list of n x s_k arrays or a pair (matrix, blkSizes); NumPy or torch, checked against n.
    The element type is kept: a complex Q_hat comes back complex, a real one as it was (NumPy lists: float64)."""
    if isinstance(Q_hat, tuple) and len(Q_hat) == 2 and getattr(Q_hat[0], "ndim", 0) == 2 and getattr(Q_hat[1], "ndim", 1) == 1:
        M, sizes = Q_hat[0], [int(s) for s in Q_hat[1]]  # (matrix, blkSizes): the second member is a flat list of sizes
    else:
        blocks = list(Q_hat)
        if not blocks:
            raise ValueError("basis_image: Q_hat has no blocks")
        for q in blocks:
            if getattr(q, "ndim", 0) != 2 or q.shape[0] != n:
                raise ValueError(f"basis_image: every block of Q_hat is an n x s_k matrix with n = {n} rows, got shape "
                                 f"{tuple(getattr(q, 'shape', ()))}")
        sizes = [int(q.shape[1]) for q in blocks]
        if _is_torch(blocks[0]):
            import torch
            M = torch.cat(list(blocks), dim=1)
        else:  # a complex Q_hat stays complex (complex128); everything else is taken as float64
            dt = np.complex128 if any(_is_complex(q) for q in blocks) else np.float64
            M = np.concatenate([np.asarray(q, dtype=dt) for q in blocks], axis=1)
    if M.shape[0] != n:
        raise ValueError(f"basis_image: Q_hat has {M.shape[0]} rows, the partition is {n} x {n}")
    if not sizes or any(s < 1 for s in sizes):
        raise ValueError(f"basis_image: block sizes must be >= 1, got {sizes}")
    if sum(sizes) != M.shape[1]:
        raise ValueError(f"basis_image: the block sizes {sizes} sum to {sum(sizes)}, Q_hat has {M.shape[1]} columns")
    if sum(sizes) > n:
        raise ValueError(f"basis_image: the block sizes sum to {sum(sizes)} > n = {n}")
    return M, sizes


def basis_image(Q_hat, P, classes=None, atol=None, ctx=None, return_route=False, _flat=False):
    """``basis_image(Q, P; atol)`` (src/diagonalize.jl:64-89) for a caller's ``Q_hat`` and a window of classes
    (``sdpsr_basis_image``): ``blks[i][k] = Q_k' 1[P == first + i] Q_k``.

    ``Q_hat``: a list of n x s_k arrays, as ``blockDiagonalize`` / ``diagonalize`` return them, or a pair
    ``(matrix, blkSizes)`` with the blocks side by side; any matrices, not only those of this library.  A complex
    ``Q_hat`` (NumPy or torch, complex64 / complex128) goes to ``sdpsr_basis_image_complex``: ``blks[i][k] =
    Q_k^H 1[P == first + i] Q_k`` as complex128, for a partition that need not be symmetric (the ``.partition`` of
    ``blockDiagonalize(..., complex=True)``); a real ``Q_hat`` needs a symmetric partition.
    ``classes = (first, count)`` (1-based, e.g. from ``class_window``); ``None``: every class.  ``atol=None``: the
    reference's ``1e-12 * n``; ``0`` clamps nothing.  Returns the window's images nested as ``blks`` of
    ``blockDiagonalize`` (``count`` rows); with ``return_route=True`` the pair ``(blks, route)``, ``route`` as
    ``SDPSR_BI_ROUTE_*`` of include/sdpsr.h.  With a device-resident partition (torch) ``Q_hat`` is taken as, or moved
    into, torch tensors of that device and the images are views of one device tensor.  The context's own block
    diagonalisation is not touched."""
    ctx = _ctx(ctx)
    n = P.shape[0]
    d = int(P.nparts)
    M, sizes = _q_hat_arg(Q_hat, n)
    first, count = (1, d) if classes is None else (int(classes[0]), int(classes[1]))
    if count < 0 or (count > 0 and (first < 1 or first + count - 1 > d)):
        raise ValueError(f"basis_image: classes = ({first}, {count}) is not a window of 1..{d}")
    S = sum(s * s for s in sizes)
    if _is_complex(M):
        return _basis_image_complex(M, sizes, P, first, count, atol, ctx, return_route, _flat)
    lab, mem = _labels_arg(P, ctx)
    route = C.c_int32(0)
    if mem == L.MEM_DEVICE:
        import torch
        Mt = M if _is_torch(M) else torch.from_numpy(np.asarray(M, dtype=np.float64))
        q = Mt.to(device=lab.device, dtype=torch.float64).t().contiguous().view(-1)  # column-major
        blks = torch.empty(max(count * S, 1), dtype=torch.float64, device=lab.device)
        ctx.wait_for(lab, q, blks)
    else:
        Mh = np.asarray(M.cpu()) if _is_torch(M) else M
        q = np.ascontiguousarray(np.asarray(Mh, dtype=np.float64).ravel(order="F"))
        blks = np.empty(max(count * S, 1), dtype=np.float64)
    sz = np.asarray(sizes, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_basis_image(ctx._h, n, _ptr(lab), d, len(sizes), _ptr(sz), _ptr(q), first, count,
                                         -1.0 if atol is None else float(atol), _ptr(blks), C.byref(route), None, mem))
    if _flat:  # basis_image_sparse: the window as the library wrote it, one flat array
        return (blks[:count * S], route.value) if return_route else blks[:count * S]
    blks = blks[:count * S].reshape(count, S)
    out = []
    for i in range(count):
        row, off = [], 0
        for s in sizes:
            b = blks[i, off:off + s * s]
            row.append(b.reshape(s, s).t() if _is_torch(b) else b.reshape(s, s, order="F"))
            off += s * s
        out.append(row)
    return (out, route.value) if return_route else out


def _basis_image_complex(M, sizes, P, first, count, atol, ctx, return_route, _flat=False):
    """``basis_image`` for a complex ``Q_hat`` (``sdpsr_basis_image_complex``): ``blks[i][k] = Q_k^H 1[P == first + i] Q_k``
    as complex128, nested like ``blockDiagonalize(..., complex=True).blks``; ``P`` need not be symmetric (the
    desymmetrized partition of the complex path is not).  On torch the blocks are views of one device tensor."""
    n, d = P.shape[0], int(P.nparts)
    S = sum(s * s for s in sizes)
    lab, mem = _labels_arg(P, ctx)
    route = C.c_int32(0)
    if mem == L.MEM_DEVICE:
        import torch
        Mt = M if _is_torch(M) else torch.from_numpy(np.asarray(M, dtype=np.complex128))
        q = Mt.to(device=lab.device, dtype=torch.complex128).t().contiguous().view(-1)  # column-major, (re, im) pairs
        blks = torch.empty(max(count * S, 1), dtype=torch.complex128, device=lab.device)
        ctx.wait_for(lab, q, blks)
    else:
        Mh = np.asarray(M.cpu()) if _is_torch(M) else M
        q = np.ascontiguousarray(np.asarray(Mh, dtype=np.complex128).ravel(order="F"))
        blks = np.empty(max(count * S, 1), dtype=np.complex128)
    sz = np.asarray(sizes, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_basis_image_complex(ctx._h, n, _ptr(lab), d, len(sizes), _ptr(sz), _ptr(q), first, count,
                                                 -1.0 if atol is None else float(atol), _ptr(blks), C.byref(route), None, mem))
    if _flat:  # basis_image_sparse: the window as the library wrote it, one flat array
        return (blks[:count * S], route.value) if return_route else blks[:count * S]
    blks = blks[:count * S].reshape(count, S)
    out = []
    for i in range(count):
        row, off = [], 0
        for s in sizes:
            b = blks[i, off:off + s * s]
            row.append(b.reshape(s, s).t() if _is_torch(b) else b.reshape(s, s, order="F"))
            off += s * s
        out.append(row)
    return (out, route.value) if return_route else out


class SparseBlocks:
    """Block images as solver triplets (``sdpsr_block_images_sparse``): the entries of window class ``i`` are
    ``[classptr[i], classptr[i + 1])`` of ``blk`` / ``row`` / ``col`` (int32, shifted by ``index_base``) and ``val``, in the
    scan order class, block, column-major inside the block.  ``sizes`` are the orders of the VIRTUAL blocks the indices
    refer to: ``s_k`` for real images, ``2 s_k`` -- the real embedding ``[Re -Im; Im Re]`` -- for complex ones.  The arrays
    are torch tensors when the input was one."""

    def __init__(self, classptr, blk, row, col, val, sizes, nnz, upper=True, index_base=0):
        self.classptr, self.blk, self.row, self.col, self.val = classptr, blk, row, col, val
        self.sizes = [int(s) for s in sizes]
        self.nnz = int(nnz)
        self.upper = bool(upper)
        self.index_base = int(index_base)

    @property
    def nclasses(self):
        return int(self.classptr.shape[0]) - 1

    @property
    def cls(self):
        """The window class of every entry (0-based plus ``index_base``), expanded from ``classptr``."""
        if _is_torch(self.classptr):
            import torch
            ids = torch.arange(self.nclasses, dtype=torch.int64, device=self.classptr.device) + self.index_base
            return torch.repeat_interleave(ids, self.classptr[1:] - self.classptr[:-1])
        return np.repeat(np.arange(self.nclasses, dtype=np.int64) + self.index_base, np.diff(self.classptr))

    def to_dense(self, mirror=False):
        """``dense[i][k]``: the virtual block as a NumPy matrix with the entries put back where they came from (for tests);
        ``mirror=True`` also writes every entry at its transposed position (the symmetric matrix an upper triangle stands for)."""
        h = [np.asarray(a.cpu()) if _is_torch(a) else np.asarray(a) for a in (self.cls, self.blk, self.row, self.col, self.val)]
        ci, bk, r, c = (a.astype(np.int64) - self.index_base for a in h[:4])
        out = [[np.zeros((s, s)) for s in self.sizes] for _ in range(self.nclasses)]
        for e in range(self.nnz):
            out[ci[e]][bk[e]][r[e], c[e]] = h[4][e]
            if mirror:
                out[ci[e]][bk[e]][c[e], r[e]] = h[4][e]
        return out


def _flat_images(blks, sizes):
    """One flat array (NumPy or torch, float64 / complex128) in the layout of ``sdpsr_block_images`` from a flat array or
    from the nested ``blks[i][k]`` that ``basis_image`` / ``blockDiagonalize`` return."""
    if _is_torch(blks):
        import torch
        return blks.reshape(-1).contiguous().to(torch.complex128 if blks.is_complex() else torch.float64)
    if isinstance(blks, np.ndarray):
        return np.ascontiguousarray(blks.reshape(-1), dtype=np.complex128 if np.iscomplexobj(blks) else np.float64)
    rows = [list(r) for r in blks]
    if any(len(r) != len(sizes) or any(tuple(b.shape) != (s, s) for b, s in zip(r, sizes)) for r in rows):
        raise ValueError(f"block_images_sparse: every class has one s_k x s_k image per block, blkSizes = {list(sizes)}")
    if rows and _is_torch(rows[0][0]):
        import torch
        cx = any(b.is_complex() for r in rows for b in r)
        return torch.cat([b.t().reshape(-1) for r in rows for b in r]).to(torch.complex128 if cx else torch.float64).contiguous()
    cx = any(np.iscomplexobj(b) for r in rows for b in r)
    dt = np.complex128 if cx else np.float64
    if not rows:
        return np.empty(0, dtype=dt)
    return np.concatenate([np.asarray(b, dtype=dt).ravel(order="F") for r in rows for b in r])


def block_images_sparse(blks, blkSizes, upper=True, tol=0.0, index_base=0, ctx=None, return_asym=False):
    """The PSD blocks as solver triplets (``sdpsr_block_images_sparse``): compacts dense block images, on the device and in
    order, into the entries ``(class, block, row, col, value)`` with ``!(|value| <= tol)``.

    ``blks``: a flat NumPy array or torch device tensor in the layout of ``sdpsr_block_images`` (class-major, then block,
    each block column-major), or the nested ``blks[i][k]`` of ``basis_image`` / ``blockDiagonalize``; ``blkSizes``: the
    ``s_k``.  Complex images (by dtype) are taken as their real embedding ``[Re -Im; Im Re]`` of order ``2 s_k``
    (docs/src/examples/ReduceAndSolveJuMP.jl:59-76 of the reference).  ``upper=True`` keeps ``row <= col`` only.  Returns
    a ``SparseBlocks``; with ``return_asym=True`` the pair ``(SparseBlocks, max |M[r,c] - M[c,r]|)`` -- what the upper
    triangle gives up."""
    ctx = _ctx(ctx)
    sizes = [int(s) for s in blkSizes]
    if not sizes or any(s < 1 for s in sizes):
        raise ValueError(f"block_images_sparse: block sizes must be >= 1, got {sizes}")
    S = sum(s * s for s in sizes)
    flat = _flat_images(blks, sizes)
    dev = _is_torch(flat)
    cx = bool(_is_complex(flat))
    total = int(flat.numel() if dev else flat.size)
    if total % S:
        raise ValueError(f"block_images_sparse: {total} elements are no multiple of sum s_k^2 = {S}")
    count = total // S
    sz = np.asarray(sizes, dtype=np.int32)
    mem = L.MEM_DEVICE if dev else L.MEM_HOST
    tri = L.TRI_UPPER if upper else L.TRI_FULL
    if dev:
        import torch
        if not flat.is_cuda:
            raise TypeError("block_images_sparse takes a torch tensor on the device (or a NumPy array)")
        classptr = torch.empty(count + 1, dtype=torch.int64, device=flat.device)
        ctx.wait_for(flat, classptr)
    else:
        classptr = np.empty(count + 1, dtype=np.int64)
    nnz, asym = C.c_int64(0), C.c_double(0.0)
    fn = ctx._lib.sdpsr_block_images_sparse
    src = _ptr(flat) if count else None
    ctx.check(fn(ctx._h, len(sizes), _ptr(sz), count, src, int(cx), tri, float(tol), int(index_base), 0, _ptr(classptr),
                 None, None, None, None, C.byref(nnz), C.byref(asym) if return_asym else None, mem))
    m = nnz.value
    if dev:
        blk, row, col = (torch.empty(m, dtype=torch.int32, device=flat.device) for _ in range(3))
        val = torch.empty(m, dtype=torch.float64, device=flat.device)
        ctx.wait_for(blk, row, col, val)
    else:
        blk, row, col = (np.empty(m, dtype=np.int32) for _ in range(3))
        val = np.empty(m, dtype=np.float64)
    if m:
        ctx.check(fn(ctx._h, len(sizes), _ptr(sz), count, src, int(cx), tri, float(tol), int(index_base), m, _ptr(classptr),
                     _ptr(blk), _ptr(row), _ptr(col), _ptr(val), C.byref(nnz), None, mem))
    out = SparseBlocks(classptr, blk, row, col, val, [2 * s if cx else s for s in sizes], m, upper, index_base)
    return (out, asym.value) if return_asym else out


def _device_partition(P, ctx):
    """``P`` with its labels on the context's device (a torch tensor at the context's label width); ``P`` itself when it
    is there already."""
    if _is_torch(P.matrix):
        return P
    import torch
    n = P.shape[0]
    flat = _lab(P.matrix, ctx)  # column-major
    signed = {8: np.uint8, 16: np.uint16 if hasattr(torch, "uint16") else np.int16, 32: np.int32}[ctx.label_width]
    t = torch.from_numpy(flat.view(signed)).to(torch.device("cuda", ctx.device))
    return Partition(P.nparts, t.view(n, n).t())  # _labels_arg reads the transposed view back as this flat buffer


def basis_image_sparse(Q_hat, P, parts=1, classes=None, atol=None, upper=True, tol=0.0, ctx=None, index_base=0):
    """``basis_image`` delivered as solver triplets: the classes (``classes = (first, count)``, default all) are cut into
    ``parts`` windows (``class_window``), each window's dense slab is made by ``basis_image`` and stays on the device, is
    compacted there (``block_images_sparse``) and only its entries are kept: peak dense memory is one slab, however large
    ``d * sum s_k^2`` is.  ``classptr`` of the result runs over all ``count`` classes.  Arguments as ``basis_image`` and
    ``block_images_sparse``; the arrays of the result are torch tensors when ``P`` is device-resident, else NumPy."""
    ctx = _ctx(ctx)
    d = int(P.nparts)
    first, count = (1, d) if classes is None else (int(classes[0]), int(classes[1]))
    if count < 0 or (count > 0 and (first < 1 or first + count - 1 > d)):
        raise ValueError(f"basis_image_sparse: classes = ({first}, {count}) is not a window of 1..{d}")
    M, sizes = _q_hat_arg(Q_hat, P.shape[0])
    cx = bool(_is_complex(M))
    to_host = not _is_torch(P.matrix)
    Pd = _device_partition(P, ctx)
    import torch
    dev = Pd.matrix.device
    if not _is_torch(M):
        M = torch.from_numpy(np.asarray(M, dtype=np.complex128 if cx else np.float64)).to(dev)
    ptr = [torch.zeros(1, dtype=torch.int64, device=dev)]
    pieces = {k: [] for k in ("blk", "row", "col", "val")}
    nnz = 0
    for j in range(int(parts)):
        f, cnt = class_window(count, parts, j)
        if cnt == 0:
            continue
        slab = basis_image((M, sizes), Pd, classes=(first + f - 1, cnt), atol=atol, ctx=ctx, _flat=True)
        sp = block_images_sparse(slab, sizes, upper=upper, tol=tol, index_base=index_base, ctx=ctx)
        del slab
        ptr.append(sp.classptr[1:] + nnz)
        nnz += sp.nnz
        for k in pieces:
            pieces[k].append(getattr(sp, k))
    cat = {k: torch.cat(v) if v else torch.empty(0, dtype=torch.float64 if k == "val" else torch.int32, device=dev) for k, v in pieces.items()}
    cp = torch.cat(ptr)
    if to_host:
        cp = cp.cpu().numpy()
        cat = {k: v.cpu().numpy() for k, v in cat.items()}
    return SparseBlocks(cp, cat["blk"], cat["row"], cat["col"], cat["val"], [2 * s if cx else s for s in sizes], nnz, upper, index_base)


def _block_diagonalize_complex(P, verbose, epsilon, ctx, retries):
    """``blockDiagonalize(ComplexF64, P)`` (src/compat.jl:46-68, src/diagonalize.jl:13-28): the
    block images are indexed by the classes of the DESYMMETRIZED partition (src/compat.jl:54-57),
    returned as ``.partition`` of the result."""
    for attempt in range(int(retries)):
        try:
            return _block_diagonalize_complex(P, verbose, epsilon, ctx, 0)
        except (NumericalInconsistency, DimensionMismatch):
            pass
    n = P.shape[0]
    lab = _lab(np.asarray(P.matrix.cpu() if _is_torch(P.matrix) else P.matrix), ctx)
    Pd = np.empty(n * n, dtype=ctx.label_dtype)
    dd = C.c_int64(0)
    nb = C.c_int32(0)
    ssq = C.c_int64(0)
    ss = C.c_int64(0)
    ctx.check(ctx._lib.sdpsr_block_diagonalize_complex(ctx._h, n, _ptr(lab), P.nparts, float(epsilon), _ptr(Pd), C.byref(dd),
                                                       C.byref(nb), C.byref(ssq), C.byref(ss), L.MEM_HOST))
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes_complex(ctx._h, _ptr(sizes)))
    d = dd.value
    blks = np.empty(2 * d * ssq.value, dtype=np.float64)
    qh = np.empty(2 * n * ss.value, dtype=np.float64)
    ctx.check(ctx._lib.sdpsr_block_images_complex(ctx._h, _ptr(blks), _ptr(qh), L.MEM_HOST))
    blks = blks.view(np.complex128).reshape(d, ssq.value)
    qh = qh.view(np.complex128).reshape(n, ss.value, order="F")
    out = []
    for i in range(d):
        row, off = [], 0
        for s in sizes:
            row.append(blks[i, off:off + s * s].reshape(s, s, order="F"))
            off += s * s
        out.append(row)
    Q, off = [], 0
    for s in sizes:
        Q.append(qh[:, off:off + s])
        off += s
    res = ComplexBlockDiagonalization([int(s) for s in sizes], out, Q, Partition(d, Pd.reshape(n, n, order="F")))
    if verbose:
        print(f"[sdpsr] blockDiagonalize over ComplexF64: blocks {res.blkSizes}, dim(desymmetrized P) = {d}")
    return res


def diagonalize(P, atol=None, ctx=None):
    """``diagonalize(Float64, P; atol)`` (src/diagonalize.jl:25-40): ``Q_hat``, a list of
    n x s_k matrices (one column per merged eigenspace of an isomorphism class)."""
    n = P.shape[0]
    atol = 1e-12 * n if atol is None else atol
    ctx = _ctx(ctx)
    lab, mem = _labels_arg(P, ctx)
    ctx.wait_for(lab)
    nb = C.c_int32(0)
    ssq = C.c_int64(0)
    ss = C.c_int64(0)
    st = ctx._lib.sdpsr_block_diagonalize(ctx._h, n, _ptr(lab), P.nparts, float(atol), C.byref(nb),
                                          C.byref(ssq), C.byref(ss), None, mem)
    if st != 3:  # diagonalize itself does not run check_block_sizes (src/compat.jl:60 does)
        ctx.check(st)
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, _ptr(sizes)))
    qh = np.empty(n * ss.value, dtype=np.float64)
    ctx.check(ctx._lib.sdpsr_q_hat(ctx._h, _ptr(qh), L.MEM_HOST))
    qh = qh.reshape(n, ss.value, order="F")
    Q, off = [], 0
    for s in sizes:
        Q.append(qh[:, off:off + s])
        off += s
    return Q


def eigen_decomposition(P, atol=None, ctx=None):
    """``eigen_decomposition(P, A; atol)`` (src/eigen_decomposition.jl:236-273): returns
    (number of eigenspaces, number of isomorphism classes) or raises."""
    n = P.shape[0]
    atol = 1e-12 * n if atol is None else atol
    ctx = _ctx(ctx)
    lab, mem = _labels_arg(P, ctx)
    ctx.wait_for(lab)
    ne = C.c_int32(0)
    nc = C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_eigen_decomposition(ctx._h, n, _ptr(lab), P.nparts, float(atol), C.byref(ne), C.byref(nc), mem))
    return ne.value, nc.value


def eigen_decomposition_batched(P, count, atol=None, values=None, ctx=None, raise_on_failure=True):
    """``count`` independent runs of ``eigen_decomposition(P, A; atol)`` on one partition
    (test/numerical_issues.jl:85-94 runs 10 000 of them): one workgroup per run on the device.
    ``values``: optional array (count, 2, dim(P)) of class values for the two generic elements of
    every run.  Returns (status, neig, nclasses) int32 arrays; raises the first failure like the
    reference would unless ``raise_on_failure`` is False."""
    n = P.shape[0]
    atol = 1e-12 * n if atol is None else atol
    ctx = _ctx(ctx)
    lab, mem = _labels_arg(P, ctx)
    ctx.wait_for(lab)
    vals = None
    if values is not None:
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(count, 2, P.nparts)
        if mem != L.MEM_HOST:
            raise ValueError("explicit values need host-resident labels")
    st = np.zeros(count, dtype=np.int32)
    ne = np.zeros(count, dtype=np.int32)
    nc = np.zeros(count, dtype=np.int32)
    rc = ctx._lib.sdpsr_eigen_decomposition_batched(ctx._h, n, _ptr(lab), P.nparts, float(atol), int(count), _ptr(vals),
                                                    _ptr(st), _ptr(ne), _ptr(nc), mem)
    if rc != 0 and (raise_on_failure or rc not in (2, 9)):
        ctx.check(rc)
    return st, ne, nc


# ---------------------------------------------------------------------------
# the reduced PSD blocks as an operator: Z(x), its adjoint, block spectra
# ---------------------------------------------------------------------------
def _flat_blocks(Z, sizes, what):
    """One flat float64 array (NumPy or torch) in the one-class layout of ``sdpsr_block_images`` -- blocks side by side, each
    column-major -- from that flat array or from a list of ``s_k x s_k`` matrices."""
    S = sum(s * s for s in sizes)
    if _is_torch(Z):
        import torch
        flat = Z.reshape(-1).contiguous().to(torch.float64)
    elif isinstance(Z, np.ndarray) and Z.ndim == 1:
        flat = np.ascontiguousarray(Z, dtype=np.float64)
    else:
        blocks = list(Z)
        if len(blocks) != len(sizes) or any(tuple(b.shape) != (s, s) for b, s in zip(blocks, sizes)):
            raise ValueError(f"{what}: one s_k x s_k matrix per block, sizes = {list(sizes)}")
        if blocks and _is_torch(blocks[0]):
            import torch
            flat = torch.cat([b.t().reshape(-1) for b in blocks]).to(torch.float64).contiguous()
        else:
            flat = np.concatenate([np.asarray(b, dtype=np.float64).ravel(order="F") for b in blocks])
    if int(flat.numel() if _is_torch(flat) else flat.size) != S:
        raise ValueError(f"{what}: {S} elements expected (sum s_k^2), sizes = {list(sizes)}")
    return flat


def _split_blocks(flat, sizes):
    """The blocks of a flat one-class array as matrices (views)."""
    out, off = [], 0
    for s in sizes:
        b = flat[off:off + s * s]
        out.append(b.reshape(s, s).t() if _is_torch(b) else b.reshape(s, s, order="F"))
        off += s * s
    return out


class BlockOperator:
    """The reduced PSD pencil ``Z_k(x) = sum_i x_i blks[i][k]`` on the device (``sdpsr_blockop_create``):
    ``sum(blkD.blks[i] .* x[i] for i = 1:dim(P))`` of docs/src/examples/ErdosRenyiThetaFunction.jl:83 and
    test/sd_problems.jl:46-52 of the reference, its adjoint ``g_i = sum_k <blks[i][k], S_k>`` -- what a first-order method
    over the reduced SDP evaluates once per iteration.

    ``sp_or_blks``: a ``SparseBlocks`` (``block_images_sparse`` / ``basis_image_sparse``), or dense images -- nested
    ``blks[i][k]``, a flat array or a torch tensor -- with ``blkSizes``; those go through ``block_images_sparse`` first
    (upper triangle, ``tol = 0``).  A context manager; ``close()`` frees the device arrays."""

    def __init__(self, sp_or_blks, blkSizes=None, ctx=None):
        self._h = None
        self.ctx = _ctx(ctx)
        sp = sp_or_blks
        if not isinstance(sp, SparseBlocks):
            if blkSizes is None:
                raise ValueError("BlockOperator: dense images need blkSizes")
            sp = block_images_sparse(sp_or_blks, blkSizes, upper=True, tol=0.0, ctx=self.ctx)
        on_dev = _is_torch(sp.val)
        arrays = (sp.classptr, sp.blk, sp.row, sp.col, sp.val)
        if on_dev:
            import torch
            if not all(a.is_cuda for a in arrays):
                raise TypeError("BlockOperator takes torch tensors on the device (or NumPy arrays)")
            want = (torch.int64, torch.int32, torch.int32, torch.int32, torch.float64)
            arrays = tuple(a.contiguous().to(t) for a, t in zip(arrays, want))
            self.ctx.wait_for(*arrays)
        else:
            want = (np.int64, np.int32, np.int32, np.int32, np.float64)
            arrays = tuple(np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, want))
        sz = np.asarray(sp.sizes, dtype=np.int32)
        nnz = int(sp.nnz)
        h = C.c_void_p()
        lib = self.ctx._lib
        st = lib.sdpsr_blockop_create(self.ctx._h, len(sz), _ptr(sz), sp.nclasses, nnz, _ptr(arrays[0]),
                                      *[(_ptr(a) if nnz else None) for a in arrays[1:]],
                                      L.TRI_UPPER if sp.upper else L.TRI_FULL, int(sp.index_base),
                                      L.MEM_DEVICE if on_dev else L.MEM_HOST, C.byref(h))
        if st == 5:  # SDPSR_BAD_ARGUMENT: malformed triplets
            raise ValueError(lib.sdpsr_last_error(self.ctx._h).decode())
        self.ctx.check(st)
        self._h = h
        d, nb, ssq, nf = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self.ctx.check(lib.sdpsr_blockop_info(self._h, C.byref(d), C.byref(nb), C.byref(ssq), C.byref(nf)))
        self.d, self.sum_sq, self.nnz_full = int(d.value), int(ssq.value), int(nf.value)
        self.sizes = [int(s) for s in sz]

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.sdpsr_blockop_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _map(self, fn, v, n_in, n_out, ctx):
        ctx = self.ctx if ctx is None else ctx
        if self._h is None:
            raise ValueError("BlockOperator: the handle is closed")
        if _is_torch(v):
            import torch
            if not v.is_cuda:
                raise TypeError("BlockOperator takes torch tensors on the device (or NumPy arrays)")
            out = torch.empty(n_out, dtype=torch.float64, device=v.device)
            ctx.wait_for(v, out)
            mem = L.MEM_DEVICE
        else:
            out = np.empty(n_out, dtype=np.float64)
            mem = L.MEM_HOST
        if int(v.numel() if _is_torch(v) else v.size) != n_in:
            raise ValueError(f"BlockOperator: {n_in} elements expected")
        ctx.check(fn(ctx._h, self._h, _ptr(v) if n_in else None, _ptr(out) if n_out else None, mem))
        return out

    def apply(self, x, flat=False, ctx=None):
        """``Z(x)``: the list of the symmetric ``Z_k``, or with ``flat=True`` the flat array in the one-class layout of
        ``sdpsr_block_images``; torch tensors when ``x`` is one."""
        if _is_torch(x):
            import torch
            x = x.reshape(-1).contiguous().to(torch.float64)
        else:
            x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        Z = self._map(self.ctx._lib.sdpsr_blockop_apply, x, self.d, self.sum_sq, ctx)
        return Z if flat else _split_blocks(Z, self.sizes)

    def adjoint(self, S, ctx=None):
        """``g_i = sum_k <blks[i][k], S_k>`` for symmetric ``S``, given as the list of blocks or flat."""
        S = _flat_blocks(S, self.sizes, "BlockOperator.adjoint")
        return self._map(self.ctx._lib.sdpsr_blockop_adjoint, S, self.sum_sq, self.d, ctx)


    def solve(self, newA, newB, newC, sense="max", rho=1.0, eps=1e-9, max_iters=20000, check_every=50, adapt_rho=False,
              nonneg=True, return_S=False, return_Y=False, raise_on_limit=False, ctx=None):
        """The reduced SDP ``max / min newC x  s.t.  newA x = newB, x >= 0, Z_k(x) PSD`` over this operator by the
        library's first-order solver (``sdpsr_sdp_solve``; the model of docs/src/examples/ReduceAndSolveJuMP.jl:40-84).
        ``newA``: r x d with independent rows (``reduced_sdp`` / ``compress_constraints``; r = 0 or ``None`` is legal),
        ``newB``: r, ``newC``: d -- NumPy arrays or torch tensors (read on the host).  Returns a ``SolveResult``: ``x``,
        ``objective``, ``status`` (``"converged"`` or ``"iteration_limit"``), the fields of ``sdpsr_sdp_info``, and on
        request ``S`` (the PSD split variable, a list of blocks) and ``Y = rho * Lambda`` (its multiplier).  Dependent rows,
        non-finite inputs, d > 4096 or a block of an order above the context's ``psd_max_order``: ``ValueError``.  ``raise_on_limit``: ``NotConverged`` instead
        of the ``"iteration_limit"`` status.  This is ADMM, not an interior-point method: see the README for what accuracy
        to expect."""
        ctx = self.ctx if ctx is None else ctx
        if self._h is None:
            raise ValueError("BlockOperator: the handle is closed")
        if sense not in ("max", "min"):
            raise ValueError("sense is 'max' or 'min'")

        def host(a):
            return np.asarray(a.detach().cpu().numpy() if _is_torch(a) else _dense(a), dtype=np.float64)

        c = np.ascontiguousarray(host(newC).reshape(-1))
        if c.size != self.d:
            raise ValueError(f"newC has {c.size} entries, the operator {self.d} classes")
        if newA is None:
            A, b = np.zeros((0, self.d), order="F"), np.zeros(0)
        else:
            A = np.asfortranarray(host(newA).reshape(-1, self.d))
            b = np.ascontiguousarray(host(newB).reshape(-1))
        r = A.shape[0]
        if b.size != r:
            raise ValueError(f"newB has {b.size} entries, newA {r} rows")
        o = L.SdpOpts(float(rho), float(eps), int(max_iters), int(check_every), 1 if adapt_rho else 0, 1 if sense == "max" else -1,
                      1 if nonneg else -1)
        info = L.SdpInfo()
        x = np.zeros(self.d)
        S = np.zeros(self.sum_sq) if return_S else None
        Y = np.zeros(self.sum_sq) if return_Y else None
        lib = ctx._lib
        st = lib.sdpsr_sdp_solve(ctx._h, self._h, r, _ptr(A) if r else None, _ptr(b) if r else None, _ptr(c), C.byref(o), _ptr(x),
                                 _ptr(S), _ptr(Y), C.byref(info), L.MEM_HOST)
        if st == 5:  # SDPSR_BAD_ARGUMENT
            raise ValueError(lib.sdpsr_last_error(ctx._h).decode())
        if st == 9 and not raise_on_limit:  # SDPSR_NOT_CONVERGED: every output is written as it stands
            st = 0
            status = "iteration_limit"
        else:
            status = "converged"
        ctx.check(st)
        return SolveResult(x, float(info.objective), status, int(info.iters), float(info.r_primal), float(info.r_dual), float(info.rho),
                           int(info.rho_changes), float(info.eq_residual), float(info.min_x), float(info.lambda_min),
                           _split_blocks(S, self.sizes) if return_S else None, _split_blocks(Y, self.sizes) if return_Y else None)


SolveResult = namedtuple("SolveResult", ["x", "objective", "status", "iters", "r_primal", "r_dual", "rho", "rho_changes", "eq_residual",
                                         "min_x", "lambda_min", "S", "Y"])


def psd_project(Z, sizes, return_lambda_min=False, ctx=None):
    """The projection of every block onto the PSD cone, ``P_k = V max(w, 0) V'`` (``sdpsr_psd_project``): ``Z`` as
    ``BlockOperator.apply`` returns it (a list of blocks or the flat array; NumPy, or torch on the device; only the lower
    triangles are read).  Returns the blocks in the form they came in (list or flat), exactly symmetric; with
    ``return_lambda_min=True`` the pair ``(P, lambda_min)`` with the smallest eigenvalue of each block.  Orders above the
    context's ``psd_max_order``: ``ValueError``."""
    ctx = _ctx(ctx)
    sizes = [int(s) for s in sizes]
    if not sizes or any(s < 1 for s in sizes):
        raise ValueError(f"psd_project: block sizes must be >= 1, got {sizes}")
    was_flat = _is_torch(Z) or (isinstance(Z, np.ndarray) and Z.ndim == 1)
    flat = _flat_blocks(Z, sizes, "psd_project")
    sz = np.asarray(sizes, dtype=np.int32)
    if _is_torch(flat):
        import torch
        if not flat.is_cuda:
            raise TypeError("psd_project takes a torch tensor on the device (or NumPy arrays)")
        P = torch.empty_like(flat)
        lm = torch.empty(len(sizes), dtype=torch.float64, device=flat.device) if return_lambda_min else None
        ctx.wait_for(flat, P)
        mem = L.MEM_DEVICE
    else:
        P = np.empty_like(flat)
        lm = np.empty(len(sizes), dtype=np.float64) if return_lambda_min else None
        mem = L.MEM_HOST
    st = ctx._lib.sdpsr_psd_project(ctx._h, len(sizes), _ptr(sz), _ptr(flat), _ptr(P), _ptr(lm), mem)
    if st == 5:  # SDPSR_BAD_ARGUMENT
        raise ValueError(ctx._lib.sdpsr_last_error(ctx._h).decode())
    ctx.check(st)
    out = P if was_flat else _split_blocks(P, sizes)
    return (out, lm) if return_lambda_min else out


ReduceAndSolveResult = namedtuple("ReduceAndSolveResult", ["jTime", "blkTime", "solveTime", "optVal", "blkSize", "originalSize", "newSize",
                                                           "solution"])


def reduce_and_solve(C_, A, b, sense="max", complex=False, limit_size=3000, ctx=None, verbose=False, retries=2, **solver):
    """``reduceAndSolve(C, A, b; objSense, verbose, complex, limitSize)`` of docs/src/examples/ReduceAndSolveJuMP.jl:10-113
    with the library's own solver in CSDP's place: ``admissible_subspace`` -> ``blockDiagonalize`` -> ``reduced_sdp`` ->
    ``basis_image_sparse`` -> ``BlockOperator`` -> ``solve``.  Returns the reference's named tuple -- ``jTime``,
    ``blkTime``, ``solveTime`` (seconds), ``optVal``, ``blkSize``, ``originalSize``, ``newSize`` -- plus ``solution``, the
    ``SolveResult``; above ``limit_size`` the zero-filled tuple the reference returns; ``None`` when ``blockDiagonalize``
    fails (``retries`` fresh generic elements first).  ``solver``: keyword arguments of ``BlockOperator.solve``.  A block
    of an order above the context's ``psd_max_order``: ``ValueError`` from the solver."""
    import time
    ctx = _ctx(ctx)
    t0 = time.perf_counter()
    P = admissible_subspace(C_, A, b, ctx=ctx, verbose=verbose)
    j_time = time.perf_counter() - t0
    n = int(P.shape[0])
    if dim(P) > limit_size:
        return ReduceAndSolveResult(j_time, 0, 0, 0, 0, n, dim(P), None)
    t0 = time.perf_counter()
    try:
        bd = blockDiagonalize(P, verbose, complex=complex, ctx=ctx, retries=retries)
    except (NumericalInconsistency, DimensionMismatch, InvalidDecompositionField):
        return None  # either random / rounding error, or complex numbers needed
    blk_time = time.perf_counter() - t0
    t0 = time.perf_counter()
    newA, newB, newC = reduced_sdp(P, A, b, C_, ctx=ctx)
    sp = basis_image_sparse(bd.Q_hat, P, ctx=ctx)
    with BlockOperator(sp, ctx=ctx) as op:
        sol = op.solve(newA, newB, newC, sense=sense, **solver)
    solve_time = time.perf_counter() - t0
    return ReduceAndSolveResult(j_time, blk_time, solve_time, sol.objective, list(bd.blkSizes), n, dim(P), sol)


def block_eigvals(Z, sizes, vectors=False, ctx=None):
    """The spectra of all blocks in one call (``sdpsr_blocks_syev``): ``Z`` as ``BlockOperator.apply`` returns it (list or
    flat; only the lower triangles are read).  Returns the list of ascending ``w_k``; with ``vectors=True`` the pair
    ``(w, V)`` with the orthonormal eigenvectors as the columns of ``V_k``."""
    ctx = _ctx(ctx)
    sizes = [int(s) for s in sizes]
    if not sizes or any(s < 1 for s in sizes):
        raise ValueError(f"block_eigvals: block sizes must be >= 1, got {sizes}")
    flat = _flat_blocks(Z, sizes, "block_eigvals")
    sz = np.asarray(sizes, dtype=np.int32)
    if _is_torch(flat):
        import torch
        if not flat.is_cuda:
            raise TypeError("block_eigvals takes a torch tensor on the device (or NumPy arrays)")
        w = torch.empty(int(sz.sum()), dtype=torch.float64, device=flat.device)
        V = torch.empty_like(flat) if vectors else None
        ctx.wait_for(flat, w)
        mem = L.MEM_DEVICE
    else:
        w = np.empty(int(sz.sum()), dtype=np.float64)
        V = np.empty_like(flat) if vectors else None
        mem = L.MEM_HOST
    ctx.check(ctx._lib.sdpsr_blocks_syev(ctx._h, len(sizes), _ptr(sz), _ptr(flat), _ptr(w), _ptr(V), mem))
    ws, off = [], 0
    for s in sizes:
        ws.append(w[off:off + s])
        off += s
    return (ws, _split_blocks(V, sizes)) if vectors else ws


BlockSpectrumCheck = namedtuple("BlockSpectrumCheck", ["full_to_blocks", "blocks_to_full", "lambda_min_full", "lambda_min_blocks",
                                                       "x", "full_spectrum", "block_spectra"])


def _directed_distance(a, b):
    """max over a of the distance to the nearest element of b (inf for an empty b, 0 for an empty a)."""
    a, b = np.asarray(a, dtype=np.float64), np.sort(np.asarray(b, dtype=np.float64))
    if a.size == 0:
        return 0.0
    if b.size == 0:
        return float("inf")
    j = np.clip(np.searchsorted(b, a), 1, b.size - 1) if b.size > 1 else np.zeros(a.size, dtype=np.int64)
    lo = np.abs(a - b[np.maximum(j - 1, 0)])
    return float(np.max(np.minimum(lo, np.abs(a - b[j]))))


def block_spectrum_check(P, bd, x=None, ctx=None):
    """The defining property of ``blockDiagonalize`` end to end: ``x -> (Z_k(x))_k`` is an algebra isomorphism, so the
    spectrum of ``X(x) = fill(P, x)`` equals, as a set, the union of the spectra of the ``Z_k(x)``.  ``bd``: a
    ``BlockDiagonalization`` or a pair ``(blks, blkSizes)``.  ``x``: ``dim(P)`` values; drawn through ``randomize`` (the
    context's seed governs) when None.  The spectrum of ``X`` comes from ``sdpsr_syev_f64``, the block spectra from
    ``BlockOperator`` and ``block_eigvals``.  Returns the two Hausdorff distances (full -> blocks, blocks -> full),
    ``lambda_min`` of both sides, ``x`` and the spectra.  Real path only: ``ValueError`` for a non-symmetric ``P``."""
    ctx = _ctx(ctx)
    lab = np.asarray(P.matrix.cpu() if _is_torch(P.matrix) else P.matrix)
    if lab.ndim != 2 or lab.shape[0] != lab.shape[1] or not np.array_equal(lab, lab.T):
        raise ValueError("block_spectrum_check: P is not symmetric (the real path needs a symmetric partition)")
    Ph = Partition(P.nparts, lab)
    blks, sizes = (bd.blks, bd.blkSizes) if hasattr(bd, "blkSizes") else bd
    if x is None:
        R = randomize(Ph, ctx=ctx)
        x = np.zeros(P.nparts, dtype=np.float64)
        x[lab[lab > 0].astype(np.int64) - 1] = R[lab > 0]
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    X = fill(Ph, x, ctx=ctx)
    n = X.shape[0]
    A = _f(X, np.float64)
    w_full, vec = np.empty(n, dtype=np.float64), np.empty(n * n, dtype=np.float64)
    ctx.check(ctx._lib.sdpsr_syev_f64(ctx._h, n, _ptr(A), _ptr(w_full), _ptr(vec), L.MEM_HOST))
    with BlockOperator(blks, sizes, ctx=ctx) as op:
        Z = op.apply(x, flat=True)
        ws = block_eigvals(Z, op.sizes, ctx=ctx)
    w_blocks = np.concatenate(ws)
    return BlockSpectrumCheck(_directed_distance(w_full, w_blocks), _directed_distance(w_blocks, w_full), float(w_full.min()),
                              float(w_blocks.min()), x, w_full, ws)
