"""The agreement of independent restarts through the C ABI: ``sdpsr_meet_keys``, ``sdpsr_agree_partitions``,
``sdpsr_agree_block_diagonalization`` and the RCCL communicator ``sdpsr_comm_*``.

``Problem.reduce_batch(restarts=R)`` returns R partitions that are equal with probability 1 - eps; ``agree_partitions``
reconciles them -- alone (``comm=None``) or with the restarts of the other ranks of a ``Comm`` (one process per GPU) -- by
their meet, the coarsest common refinement (``refine!``, src/partitions.jl:62-66, folded over the valid restarts).
``parallel.py`` keeps the ``torch.distributed`` form of the same step; the slot multipliers are shared with it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .api import Partition, _check_torch_labels, _ctx, _is_torch, _lab, _labels_arg, _ptr
from .parallel import _slot_multiplier as slot_multiplier  # noqa: F401  (m(k) of include/sdpsr.h)

# statuses after which a restart's P_out is a partition: OK and the randomized failures of blockDiagonalize
VALID_STATUSES = (0, 2, 3)


class Comm:
    """One rank's handle of an RCCL communicator (``sdpsr_comm_create``; one process per GPU).  Every rank must make the same
    sequence of collective calls; the library adds no time-out of its own."""

    @staticmethod
    def unique_id():
        """128 bytes one rank creates and the caller distributes to the others (``sdpsr_comm_unique_id``)."""
        buf = C.create_string_buffer(128)
        st = L.load_library().sdpsr_comm_unique_id(C.cast(buf, C.c_void_p))
        if st != 0:
            raise RuntimeError(f"sdpsr_comm_unique_id failed: {L.STATUS.get(st, st)} (can librccl.so.1 be opened?)")
        return buf.raw

    def __init__(self, world, rank, unique_id, ctx=None):
        self.ctx = _ctx(ctx)
        if len(unique_id) != 128:
            raise ValueError("the unique id has 128 bytes")
        h = C.c_void_p()
        self._h = None
        self.ctx.check(self.ctx._lib.sdpsr_comm_create(self.ctx._h, int(world), int(rank), C.c_char_p(bytes(unique_id)), C.byref(h)))
        self._h = h

    @property
    def rank(self):
        return int(self.ctx._lib.sdpsr_comm_rank(self._h))

    @property
    def world(self):
        return int(self.ctx._lib.sdpsr_comm_world(self._h))

    def broadcast(self, buf, root=0):
        """``buf`` (a contiguous NumPy array or torch CUDA tensor, same size on every rank) of rank ``root`` to every rank, in
        place: the winner's ``Q_hat``."""
        if _is_torch(buf):
            if not buf.is_cuda or not buf.is_contiguous():
                raise TypeError("broadcast takes a contiguous CUDA tensor")
            nbytes, mem = buf.numel() * buf.element_size(), L.MEM_DEVICE
            self.ctx.wait_for(buf)
        else:
            if not isinstance(buf, np.ndarray) or not (buf.flags.c_contiguous or buf.flags.f_contiguous) or not buf.flags.writeable:
                raise TypeError("broadcast takes a contiguous writable NumPy array")
            nbytes, mem = buf.nbytes, L.MEM_HOST
        self.ctx.check(self.ctx._lib.sdpsr_comm_broadcast(self.ctx._h, self._h, _ptr(buf), nbytes, int(root), mem))
        return buf

    def close(self):
        """Before the context it was created on is closed."""
        if getattr(self, "_h", None):
            self.ctx._lib.sdpsr_comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _flat_arrays(parts, ctx):
    """The label arrays of ``parts`` as flat arrays at the context's width, and their memory space.  A flat NumPy array at the
    context's own dtype and a torch tensor are the caller's storage; everything else is a copy."""
    arrays, mems = [], set()
    for p in parts:
        if isinstance(p, Partition):
            a, mem = _labels_arg(p, ctx)
            a = a.clone() if _is_torch(a) else a.copy()  # (a Partition given is never written)
        elif _is_torch(p):
            _check_torch_labels(p, ctx)
            if not p.is_cuda or not p.is_contiguous():
                raise TypeError("a torch label array must be a contiguous CUDA tensor")
            a, mem = p.view(-1), L.MEM_DEVICE
        else:
            src = np.asarray(p)
            own = src.dtype == ctx.label_dtype and src.ndim == 1 and src.flags.c_contiguous and src.flags.writeable
            a, mem = (src if own else _lab(src, ctx).copy()), L.MEM_HOST
        arrays.append(a)
        mems.add(mem)
    if len(mems) != 1:
        raise TypeError("the label arrays of one call live in one memory space")
    sizes = {(a.numel() if _is_torch(a) else a.size) for a in arrays}
    if len(sizes) != 1:
        raise ValueError("the label arrays of one call have one length")
    return arrays, mems.pop()


def _valid_arg(valid, R):
    if valid is None:
        return None
    if len(valid) != R:
        raise ValueError(f"{len(valid)} validity flags for {R} restarts")
    return (C.c_int32 * R)(*[1 if v else 0 for v in valid])


def meet_keys(arrays, first_slot=0, valid=None, ctx=None):
    """``sdpsr_meet_keys``: keys[e] = sum_i arrays[i][e] * m(first_slot + i) mod 2^64 over the valid arrays, one streaming
    kernel.  ``arrays``: flat NumPy arrays (returns a ``np.uint64`` array) or flat torch CUDA tensors (returns an int64 CUDA
    tensor) at the context's label width.  A caller with a transport of its own sums the ranks' keys (wrapping) and hands
    the sum to ``relabel_keys``."""
    ctx = _ctx(ctx)
    flats, mem = _flat_arrays(arrays, ctx)
    R = len(flats)
    ptrs = (C.c_void_p * R)(*[_ptr(a).value for a in flats])
    if mem == L.MEM_DEVICE:
        import torch
        n = flats[0].numel()
        keys = torch.empty(n, dtype=torch.int64, device=flats[0].device)
        ctx.wait_for(*flats)
    else:
        n = flats[0].size
        keys = np.empty(n, dtype=np.uint64)
    ctx.check(ctx._lib.sdpsr_meet_keys(ctx._h, R, C.cast(ptrs, C.c_void_p), C.cast(_valid_arg(valid, R), C.c_void_p), n, int(first_slot),
                                       _ptr(keys), mem))
    return keys


def agree_partitions(parts, comm=None, valid=None, ctx=None):
    """``sdpsr_agree_partitions`` over the restarts ``parts`` of this process and, with ``comm``, of every other rank
    (collective).  ``parts``: ``Partition`` s, flat NumPy label arrays or flat torch CUDA tensors at the context's label width;
    ``valid[i]`` false: restart i holds no partition (its status was not in ``VALID_STATUSES``) -- it is not read and receives
    the result.  Returns ``(met, Partition)``: ``met`` False -- every restart of every rank agrees, the Partition is the first
    one given; ``met`` True -- the Partition is the meet of the valid restarts, and NumPy arrays given at the context's own
    dtype hold it too.  For torch tensors: updated in place, returns ``(met, dim)``.  Raises ``LabelOverflow`` when the meet has
    more classes than the label width holds (nothing is written then)."""
    ctx = _ctx(comm.ctx if (ctx is None and comm is not None) else ctx)
    parts = list(parts)
    flats, mem = _flat_arrays(parts, ctx)
    R = len(flats)
    ptrs = (C.c_void_p * R)(*[_ptr(a).value for a in flats])
    n = flats[0].numel() if mem == L.MEM_DEVICE else flats[0].size
    if mem == L.MEM_DEVICE:
        ctx.wait_for(*flats)
    dim, met = C.c_int64(-1), C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_agree_partitions(ctx._h, comm._h if comm is not None else None, R, C.cast(ptrs, C.c_void_p),
                                              C.cast(_valid_arg(valid, R), C.c_void_p), n, C.byref(dim), C.byref(met), mem))
    first = next(i for i in range(R) if valid is None or valid[i])
    if mem == L.MEM_DEVICE and not isinstance(parts[0], Partition):
        return bool(met.value), (int(dim.value) if met.value else int(flats[first].long().max().item()))  # (canonical labels: the largest is dim)
    if not met.value:
        p = parts[first]
        return False, (p if isinstance(p, Partition) else Partition(int(np.asarray(flats[first]).max()), flats[first]))
    if isinstance(parts[0], Partition):
        shape = parts[0].shape
        if _is_torch(flats[0]):
            n0 = shape[0]
            return True, Partition(dim.value, flats[0].view(shape[1], n0).t())
        return True, Partition(dim.value, flats[0].reshape(shape, order="F"))
    return True, Partition(dim.value, flats[0])


def agree_block_diagonalization(status, blk_sizes, comm=None, ctx=None, capacity=65536):
    """``sdpsr_agree_block_diagonalization``: the lowest rank whose ``status`` is 0 wins and every rank receives its
    ``blkSizes`` (collective with ``comm``; alone, the winner is this process or nobody).  Returns ``(winner, sizes)``;
    ``(-1, None)`` when every rank failed -- the caller retries with fresh draws.  ``capacity`` (the same on every rank) bounds
    the number of block sizes received.  The winner's ``Q_hat`` travels with ``Comm.broadcast``."""
    ctx = _ctx(comm.ctx if (ctx is None and comm is not None) else ctx)
    mine = np.ascontiguousarray(blk_sizes if blk_sizes is not None else [], dtype=np.int32)
    out = np.zeros(max(int(capacity), 1), dtype=np.int32)
    w, nb = C.c_int32(-2), C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_agree_block_diagonalization(ctx._h, comm._h if comm is not None else None, int(status), mine.size,
                                                         _ptr(mine) if mine.size else None, C.byref(w), C.byref(nb), _ptr(out), int(capacity)))
    if w.value < 0:
        return -1, None
    return int(w.value), [int(x) for x in out[:nb.value]]
