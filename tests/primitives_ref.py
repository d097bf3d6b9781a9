"""NumPy ports (uint64 arithmetic with wrap-around) of what the element-wise kernels behind the AbstractPartition primitives and the
full-matrix channel gathers compute, for tests/test_gpu_primitives.py; held against csrc/sdpsr_hash.h value for value by
tests/test_primitives_ref_cpu.py.  Nothing here touches the library.

    class_bits(key, l)          sdpsr_class_bits
    class_uniform(key, l)       sdpsr_class_uniform (label 0 -> 0.0, as every kernel has it)
    class_i8(bits, t)           sdpsr_class_i8: byte t of the bits, signed
    class_small(bits, t, vmax)  sdpsr_class_small: byte t of the bits, scaled to [-vmax, vmax]
    clamp_round(a, atol, mode)  sdpsr_clamp_round under round_scale(atol, mode) (oracle.clamp_round has both rules)
    checksum(labels)            the two words of sdpsr_partition_checksum
    probe_weights(key, n)       w(e) of the symmetry probe of the projection's dot products

GRID_THREADS is the one hand-copied constant: the threads of the largest launch grid_for() of csrc/kernel_util.h gives (2048
workgroups of 256); a kernel with more work items than that relies on its grid-stride loop."""
import numpy as np

import sdpsr_oracle
from module_kernels_ref import GOLDEN, M64, class_uniform, fmix64  # noqa: F401  (class_uniform is part of this module's surface)
from refine_source_ref import round_scale  # noqa: F401

GRID_THREADS = 2048 * 256
LEN_W = 3 * GRID_THREADS + 77   # threads below 77 make four trips of a grid-stride loop, the rest three
LEN_P = 5 * GRID_THREADS + 77   # proj_coef_kernel: the unrolled body once, its tail once (threads below 77: twice)
SMALL_LENS = (1, 63, 64, 65, 255, 256, 257)  # a ragged wave, a ragged workgroup
PROBE_XOR = 0x5DEECE66D1CE4E5B
U53 = 2.0 ** -53


def class_bits(key, labels):
    lab = np.asarray(labels, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return fmix64(np.uint64(key & M64) + np.uint64(GOLDEN) * lab)


def class_i8(bits, t):
    return ((np.asarray(bits, dtype=np.uint64) >> np.uint64(8 * t)) & np.uint64(0xFF)).astype(np.uint8).view(np.int8)


def class_small(bits, t, vmax):
    """Byte t of the bits, for EVERY t in 0 .. 7: (b (2 vmax + 1) >> 8) - vmax."""
    b = ((np.asarray(bits, dtype=np.uint64) >> np.uint64(8 * t)) & np.uint64(0xFF)).astype(np.int64)
    return ((b * (2 * vmax + 1)) >> 8) - vmax


def clamp_round(a, atol, round_mode="nearest"):
    return sdpsr_oracle.clamp_round(a, atol=atol, round_mode=round_mode)


def checksum(labels):
    """(h1, h2) of flat labels: sums over the entries e of functions of (label + 1, e), modulo 2^64."""
    lab = np.asarray(labels).reshape(-1)
    e = np.arange(lab.size, dtype=np.uint64)
    l = lab.astype(np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        h1 = int((l * (e * np.uint64(GOLDEN) + np.uint64(0xD1342543DE82EF95))).sum(dtype=np.uint64))
        h2 = int(((l * l + np.uint64(0x27D4EB2F165667C5)) *
                  ((e ^ (e >> np.uint64(13))) * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(0x94D049BB133111EB))).sum(dtype=np.uint64))
    return h1, h2


def probe_weight_ints(key, n, e=None):
    """2^53 w(e) as int64: (fmix64(wkey + e) >> 11) - (fmix64(wkey + eT) >> 11), eT the index of the transposed entry."""
    e = np.arange(n * n, dtype=np.uint64) if e is None else np.asarray(e, dtype=np.uint64)
    j, i = e // np.uint64(n), e % np.uint64(n)
    et = j + i * np.uint64(n)
    wkey = np.uint64((key ^ PROBE_XOR) & M64)
    with np.errstate(over="ignore"):
        a, b = fmix64(wkey + e) >> np.uint64(11), fmix64(wkey + et) >> np.uint64(11)
    return a.astype(np.int64) - b.astype(np.int64)


def probe_weights(key, n, e=None):
    """w(e) as the kernel forms it: the difference of two 53-bit integers (exact in float64), times 2^-53."""
    return probe_weight_ints(key, n, e).astype(np.float64) * U53


def uniform_ints(key, labels):
    """2^53 class_uniform(key, l) as int64 (0 for label 0)."""
    lab = np.asarray(labels, dtype=np.uint64)
    return np.where(lab == 0, np.uint64(0), class_bits(key, lab) >> np.uint64(11)).astype(np.int64)


def exact_dot_ints(ui, xi):
    """(sum_e ui[e] xi[e], sum_e |ui[e] xi[e]|) as Python integers, for int64 ui with |ui| <= 4 and int64 |xi| < 2^53."""
    ui, xi = np.asarray(ui, dtype=np.int64), np.asarray(xi, dtype=np.int64)
    assert np.abs(ui).max(initial=0) <= 4 and len(ui) < 2 ** 31 and np.abs(xi).max(initial=0) < 2 ** 53
    hi, lo = xi >> 27, xi & ((1 << 27) - 1)  # xi = hi 2^27 + lo; |ui hi|, |ui lo| < 2^29: int64 sums of < 2^31 terms are exact
    s = (int((ui * hi).sum()) << 27) + int((ui * lo).sum())
    ax = np.abs(xi)
    sa = (int((np.abs(ui) * (ax >> 27)).sum()) << 27) + int((np.abs(ui) * (ax & ((1 << 27) - 1))).sum())
    return s, sa


def scaled(s, q=0):
    """The Python integer s in units of 2^-(53 + q) as a float64, rounded once."""
    return s / 2 ** (53 + q)


def integer_basis(U, q=0):
    """U 2^q as int64, asserting that it is one (the scaling is exact)."""
    ui = np.ldexp(U, q).astype(np.int64)
    assert np.array_equal(np.ldexp(ui.astype(np.float64), -q), U)
    return ui


def dot_bound(length, sum_abs):
    """The a-priori bound of a float64 dot product of `length` terms summed in ANY order, with or without fma:
    gamma_len <= len u / (1 - len u) <= 2 len u for len u <= 1/2, u = 2^-53."""
    assert length * U53 <= 0.5
    return 2.0 * length * U53 * sum_abs


def tie_values():
    """Doubles whose mantissa, scaled by 1e7 = 2^7 * 78125, is an exact half-integer: (2 j + 1) / 256 * 2^e, j = 64 .. 127
    (mantissa (2 j + 1) / 256 in [0.5, 1), times 1e7 = (2 j + 1) * 78125 / 2: odd over two)."""
    j = np.arange(64, 128)
    m = (2 * j + 1) / 256.0
    return np.concatenate([np.ldexp(m, e) for e in (-20, -3, 0, 1, 9)])


def clamp_values(length, atol, seed=3):
    """`length` finite doubles for sdpsr_clamp_round: the mix of test_clamp_round_and_projection, exact ties of the scaled mantissa and
    their neighbours, values one ulp either side of atol, +-0.0, mantissas that round up to 1.0 -- planted at the front, where a second
    and a third trip of the grid-stride loop read, and at the end (at LEN_W: the end of the third trip and all of the fourth)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(length) * 10.0 ** rng.integers(-12, 6, length)
    ties = tie_values()
    near_one = np.ldexp(1.0 - np.array([1, 3, 40, 1999]) * 2.0 ** -33, np.array([-9, 0, 3, 5]))
    edge = np.array([0.0625, 1e-10, -1e-9, 0.0, -0.0, atol, np.nextafter(atol, 0.0), np.nextafter(atol, 1.0), -atol, -np.nextafter(atol, 0.0),
                     -np.nextafter(atol, 1.0), 0.99999995, 0.99999994999, 5e-324, 1e300, -1e-300])
    plant = np.concatenate([ties, -ties, np.nextafter(ties, 0.0), np.nextafter(ties, 9e9), near_one, -near_one, edge])
    for start in (0, GRID_THREADS + 5, 2 * GRID_THREADS + 5, length - len(plant)):
        if 0 <= start and start + len(plant) <= length:
            a[start:start + len(plant)] = plant
    if length < len(plant):
        a[:] = plant[np.linspace(0, len(plant) - 1, length).astype(np.int64)]  # (a sample across every kind of planted value)
    return a


# ---- the symmetry probe's planted asymmetries ----
PROBE_BASE_KEY = 0x5DEECE66D1234567


def probe_pairs(n):
    """The (i, j), i != j, whose U entry a probe case perturbs: one in the last row and, where the matrix has more entries than
    one trip of the grid-stride loop takes, one in a column only a later trip reaches."""
    pairs = [(n - 1, n // 3)] if n > 1 else []
    if n * n > GRID_THREADS + n:
        j = GRID_THREADS // n + 2
        pairs.append((7, j))
        assert GRID_THREADS <= 7 + j * n < 2 * GRID_THREADS and j < n
    return pairs


def probe_key(n):
    """The first key PROBE_BASE_KEY + k under which |w_ij - w_ji| = 2 |w(i + j n)| > 0.1 at every pair of probe_pairs(n)."""
    for k in range(64):
        key = PROBE_BASE_KEY + k
        if all(2.0 * abs(probe_weights(key, n, [i + j * n])[0]) > 0.1 for i, j in probe_pairs(n)):
            return key
    raise AssertionError("no key")
