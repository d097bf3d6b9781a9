"""NumPy reference of a label-width conversion (Partition{T}, src/partitions.jl:6-11): the values are unchanged, so the array
at another width is ``astype``; a value the target type cannot hold is the reference's InexactError.  Shared by
test_label_width_cpu.py (which checks it on the edge values) and test_gpu_label_width.py (which checks the library against it)."""
import numpy as np

DTYPES = {8: np.dtype(np.uint8), 16: np.dtype(np.uint16), 32: np.dtype(np.uint32)}


class Inexact(Exception):
    """A label does not fit the target width."""


def typemax(bits):
    return (1 << bits) - 1


def convert_reference(a, bits):
    """``a`` (any unsigned label dtype) at ``bits`` bits per label; raises ``Inexact`` when a value does not fit."""
    a = np.asarray(a)
    if a.size and int(a.max()) > typemax(bits):
        raise Inexact(f"{int(a.max())} does not fit {bits} bits")
    return a.astype(DTYPES[bits])


def random_labels(len_, bits, seed):
    """Random labels that fit ``bits`` bits, with 0 and the type's maximum at the first, the last and a middle position
    (as far as ``len_`` has them: first wins over last, the maximum over 0)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, typemax(bits) + 1, size=len_, dtype=np.uint64)
    edge = [typemax(bits), 0, typemax(bits)]
    for pos, v in zip((len_ - 1, len_ // 2, 0), edge):
        a[pos] = v
    if len_ >= 5:
        a[1], a[len_ - 2] = 0, 0
    return a
