"""The ports of tests/primitives_ref.py against csrc/sdpsr_hash.h compiled for the host, value for value, without a GPU; the one
hand-copied launch constant against csrc/kernel_util.h; the contracts of the inputs tests/test_gpu_primitives.py builds from them."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import primitives_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc")

SRC = r'''
#include <stdio.h>
#include <string.h>
#include "sdpsr_hash.h"
typedef unsigned long long ull;
int main(int argc, char** argv) {
  char op[16]; ull key, v; int n, vmax; double atol, sc;
  if (scanf("%15s", op) != 1) return 1;
  if (!strcmp(op, "bits")) {          /* key n, then n labels: class_bits, class_uniform (as bits), class_i8 of every byte */
    if (scanf("%llu %d", &key, &n) != 2) return 1;
    for (int k = 0; k < n; ++k) {
      if (scanf("%llu", &v) != 1) return 1;
      ull b = sdpsr_class_bits(key, (uint32_t)v); double u = sdpsr_class_uniform(key, (uint32_t)v); ull ub; memcpy(&ub, &u, 8);
      printf("%llu %llu", b, ub);
      for (int t = 0; t < 8; ++t) printf(" %d", sdpsr_class_i8(b, t));
      printf("\n");
    }
  } else if (!strcmp(op, "small")) {  /* vmax n, then n words: class_small of every byte */
    if (scanf("%d %d", &vmax, &n) != 2) return 1;
    for (int k = 0; k < n; ++k) {
      if (scanf("%llu", &v) != 1) return 1;
      for (int t = 0; t < 8; ++t) printf("%d ", sdpsr_class_small(v, t, vmax));
      printf("\n");
    }
  } else if (!strcmp(op, "clamp")) {  /* atol scale n, then n doubles as bits: clamp_round as bits */
    if (scanf("%lf %lf %d", &atol, &sc, &n) != 3) return 1;
    for (int k = 0; k < n; ++k) {
      if (scanf("%llu", &v) != 1) return 1;
      double a; memcpy(&a, &v, 8); double y = sdpsr_clamp_round(a, atol, sc); ull yb; memcpy(&yb, &y, 8);
      printf("%llu\n", yb);
    }
  } else if (!strcmp(op, "fmix")) {   /* n, then n words: sdpsr_fmix64 */
    if (scanf("%d", &n) != 1) return 1;
    for (int k = 0; k < n; ++k) { if (scanf("%llu", &v) != 1) return 1; printf("%llu\n", (ull)sdpsr_fmix64(v)); }
  } else return 2;
  return 0;
}
'''


@pytest.fixture(scope="module")
def header():
    """run(op, head, words) -> the program's output as a list of lines of integers."""
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(SRC)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-O2", "-I", CSRC, os.path.join(d, "t.cpp"), "-o", exe])

        def run(op, head, words):
            text = f"{op} {head} {len(words)}\n" + "\n".join(str(int(w)) for w in words) + "\n"
            out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
            return [[int(w) for w in line.split()] for line in out.strip().split("\n")]
        yield run


def _words(seed, count):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 64, size=count, dtype=np.uint64)
    w[:6] = [0, 1, P.M64, 1 << 63, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F]
    return w


def test_grid_threads_is_the_cap_of_grid_for():
    txt = open(os.path.join(CSRC, "kernel_util.h")).read()
    m = re.search(r"grid_for\(int64_t work_items, int block, int max_blocks = (\d+) \* (\d+)\)", txt)
    assert m, "grid_for's signature moved"
    assert int(m.group(1)) * int(m.group(2)) == 2048
    assert P.GRID_THREADS == 2048 * 256 == 524288
    assert P.LEN_W == 3 * 524288 + 77 and P.LEN_P == 5 * 524288 + 77


def test_fmix_and_class_draws_match_the_header(header):
    w = _words(1, 3000)
    got = np.array([r[0] for r in header("fmix", "", w)], dtype=np.uint64)
    assert np.array_equal(got, P.fmix64(w))
    labels = np.concatenate([np.arange(0, 300), np.array([2047, 2048, 2049, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]),
                             np.random.default_rng(2).integers(1, 2 ** 32, size=2000)]).astype(np.uint64)
    for key in (0, 1, P.PROBE_BASE_KEY, P.M64, 0x8000000000000000):
        rows = header("bits", f"{key}", labels)
        bits = np.array([r[0] for r in rows], dtype=np.uint64)
        assert np.array_equal(bits, P.class_bits(key, labels))
        uni = np.array([r[1] for r in rows], dtype=np.uint64).view(np.float64)
        port = P.class_uniform(key, labels)
        assert np.array_equal(uni[1:], port[1:]) and port[0] == 0.0  # (label 0 carries no value in the port; no kernel draws it)
        assert np.array_equal(P.uniform_ints(key, labels)[1:].astype(np.float64) * P.U53, uni[1:])
        assert ((uni >= 0) & (uni < 1)).all()
        for t in range(8):
            assert np.array_equal(np.array([r[2 + t] for r in rows]), P.class_i8(bits, t).astype(np.int64)), (key, t)


def test_class_small_matches_the_header_at_every_byte_value(header):
    """Every byte value in every position t, the other seven bytes random; vmax 1, 64, 127."""
    rng = np.random.default_rng(5)
    words = []
    for t in range(8):
        for b in range(256):
            noise = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
            words.append((noise & ~(0xFF << (8 * t)) & P.M64) | (b << (8 * t)))
    words = np.array(words + list(_words(6, 500)), dtype=np.uint64)
    for vmax in (1, 64, 127):
        rows = np.array(header("small", f"{vmax}", words))
        for t in range(8):
            port = P.class_small(words, t, vmax)
            assert np.array_equal(rows[:, t], port), (vmax, t)
            own = port[256 * t:256 * (t + 1)]  # byte t running over 0 .. 255
            assert own.min() == -vmax and own.max() == vmax and len(np.unique(own)) == 2 * vmax + 1 and (np.diff(own) >= 0).all()


def test_clamp_round_matches_the_header_in_both_modes(header):
    for atol in (2.0 ** -26, 1e-3, 1e-12):
        vals = np.concatenate([P.clamp_values(6000, atol), P.tie_values(), -P.tie_values()])
        for mode in ("nearest", "trunc"):
            sc = P.round_scale(atol, mode)
            got = np.array([r[0] for r in header("clamp", f"{atol!r} {sc!r}", vals.view(np.uint64))], dtype=np.uint64)
            want = P.clamp_round(vals, atol, mode)
            bad = np.flatnonzero(got != want.view(np.uint64))
            assert len(bad) == 0, (atol, mode, vals[bad[:5]], got.view(np.float64)[bad[:5]], want[bad[:5]])


def test_tie_values_are_exact_ties_and_the_rules_part_on_them():
    t = P.tie_values()
    assert len(t) == 5 * 64
    sm = 1e7 * np.frexp(t)[0]
    assert np.array_equal(sm - np.floor(sm), np.full(len(t), 0.5))  # exact half-integers: 1e7 m is exact (24 + 8 bits)
    near, trunc = P.clamp_round(t, 2.0 ** -26, "nearest"), P.clamp_round(t, 2.0 ** -26, "trunc")
    k_near, k_trunc = np.rint(1e7 * np.frexp(near)[0]), np.rint(1e7 * np.frexp(trunc)[0])
    assert np.array_equal(k_near % 2, np.zeros(len(t)))  # ties to even
    assert np.array_equal(k_trunc, np.floor(sm))
    vals = P.clamp_values(P.GRID_THREADS + 2000, 2.0 ** -26)
    assert np.isfinite(vals).all()
    for start in (0, P.GRID_THREADS + 5):
        assert np.array_equal(vals[start:start + len(t)], t)  # the ties sit where a first and a second trip read ...
    assert vals[-1] == -1e-300 and vals[-16] == 0.0625  # ... and the planted block ends the array


def test_checksum_port_against_a_plain_loop():
    rng = np.random.default_rng(8)
    lab = rng.integers(0, 2 ** 32, size=9001, dtype=np.uint64).astype(np.uint32)
    h1 = h2 = 0
    for e, l in enumerate(int(v) + 1 for v in lab):
        h1 += l * ((e * 0x9E3779B97F4A7C15 + 0xD1342543DE82EF95) & P.M64)
        h2 += ((l * l + 0x27D4EB2F165667C5) & P.M64) * ((((e ^ (e >> 13)) * 0xBF58476D1CE4E5B9) + 0x94D049BB133111EB) & P.M64)
    assert P.checksum(lab) == (h1 & P.M64, h2 & P.M64)
    lab2 = lab.copy()
    lab2[-1] ^= 1
    assert P.checksum(lab2)[0] != P.checksum(lab)[0] and P.checksum(lab2)[1] != P.checksum(lab)[1]


def test_probe_weights_port(header):
    """w(e) from the header's fmix64, entry by entry; antisymmetry (W - W' has a zero diagonal and w_ij = -w_ji), which is what makes
    the probe of a symmetric U vanish up to rounding."""
    for n, key in ((1, 5), (16, P.PROBE_BASE_KEY), (57, P.M64)):
        e = np.arange(n * n, dtype=np.uint64)
        wkey = (key ^ 0x5DEECE66D1CE4E5B) & P.M64
        et = (e // np.uint64(n)) + (e % np.uint64(n)) * np.uint64(n)
        with np.errstate(over="ignore"):
            fa = np.array([r[0] for r in header("fmix", "", np.uint64(wkey) + e)], dtype=np.uint64)
            fb = np.array([r[0] for r in header("fmix", "", np.uint64(wkey) + et)], dtype=np.uint64)
        w = ((fa >> np.uint64(11)).astype(np.float64) - (fb >> np.uint64(11)).astype(np.float64)) * (1.0 / 9007199254740992.0)
        port = P.probe_weights(key, n)
        assert np.array_equal(w, port)
        W = port.reshape(n, n, order="F")
        assert np.array_equal(W, -W.T) and not W.diagonal().any()


def test_probe_keys_make_the_planted_pairs_visible():
    for n in (16, 57, 1620):
        key = P.probe_key(n)
        pairs = P.probe_pairs(n)
        assert len(pairs) == (2 if n == 1620 else 1) and all(i != j for i, j in pairs) and pairs[0][0] == n - 1
        for i, j in pairs:
            w_ij, w_ji = P.probe_weights(key, n, [i + j * n])[0], P.probe_weights(key, n, [j + i * n])[0]
            assert abs(w_ij - w_ji) > 0.1
    assert P.probe_pairs(1) == []
    i, j = P.probe_pairs(1620)[1]
    assert P.GRID_THREADS <= i + j * 1620 < 2 * P.GRID_THREADS  # only a second trip reaches it
    assert 1620 * 1620 > 5 * P.GRID_THREADS


def test_exact_dot_and_its_bound():
    rng = np.random.default_rng(4)
    n = 5000
    U = rng.choice([-2.0, -1.0, 1.0, 2.0], size=n)
    xi = rng.integers(-2 ** 53 + 1, 2 ** 53, size=n)
    s, sa = P.exact_dot_ints(P.integer_basis(U), xi)
    assert s == sum(int(u) * int(x) for u, x in zip(U, xi)) and sa == sum(abs(int(u) * int(x)) for u, x in zip(U, xi))
    assert np.array_equal(P.integer_basis(U * 2.0 ** -24, 24), U.astype(np.int64)) and P.scaled(3 << 20, 24) == 3.0 * 2.0 ** -57
    with pytest.raises(AssertionError):
        P.integer_basis(np.array([0.3]))
    # one dropped entry of a LEN_P dot product moves it by ~1 / len relative; the bound is 2 len u
    assert P.dot_bound(P.LEN_P, 1.0) < 6e-10 and 1.0 / P.LEN_P > 100 * P.dot_bound(P.LEN_P, 1.0)
