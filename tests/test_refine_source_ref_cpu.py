"""The reference of tests/test_gpu_refine_sources.py against itself and against sdpsr_hash.h, without a GPU: the grouping against a
plain scan, the NumPy ports of sdpsr_round_key / sdpsr_class_uniform against the header compiled for the host, and the generators'
own contracts (exact projections, margins around the rounding rule's switch points and atol, the planted edge values)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import refine_source_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_cases():
    yield R.make_case("pair", 9, packed=1, lab_packed=1, seed=1)
    yield R.make_case("pair", 7, packed=0, lab_packed=0, seed=2)
    for packed, lab_packed in ((1, 1), (1, 0), (0, 0)):
        yield R.make_case("proj", 11, r=2, packed=packed, lab_packed=lab_packed, seed=3, classes=6)
        yield R.make_case("chan_i32", 11, T=3, packed=packed, lab_packed=lab_packed, seed=4, classes=6)
        yield R.make_case("chan_f32", 11, T=2, packed=packed, lab_packed=lab_packed, seed=5, classes=6)
    yield R.make_case("joint", 13, T=4, r=3, seed=6, classes=6, round_mode="trunc")
    yield R.make_planted_case("joint", 21, "nearest", seed=7)
    yield R.make_planted_case("proj", 21, "trunc", seed=8)
    yield R.make_count_case("chan_i32", 120, 50, seed=9, dense_chunk=40, last_alone=True)
    yield R.make_count_case("pair", 120, 50, seed=10)


def test_grouping_matches_a_plain_scan():
    count = 0
    for case in _small_cases():
        cols, zero = R.key_columns(case)
        lab, nparts, first = R.canonical(cols, zero)
        lab2, nparts2, first2 = R.scan_reference(cols, zero)
        assert nparts == nparts2 and np.array_equal(lab, lab2) and np.array_equal(first, first2), case["kind"]
        assert zero.any() and nparts >= 2
        count += 1
    assert count == 16


def test_count_cases_have_the_class_count_asked_for():
    for kind in ("chan_i32", "joint", "pair"):
        for ncl, kw in ((1024, {}), (1025, {}), (3073, {}), (700, dict(dense_chunk=600)), (40, dict(last_alone=True))):
            case = R.make_count_case(kind, 257, ncl, seed=ncl, **kw)
            lab, nparts, first = R.refine_reference(case)
            assert nparts == ncl
            if kw.get("dense_chunk"):
                assert len(np.unique(lab[:2048])) >= 600  # more than half the slots of the workgroup's table from one chunk
            if kw.get("last_alone"):
                assert int(first[-1]) == len(lab) - 1 and int((lab == lab[-1]).sum()) == 1
    many = R.make_count_case("chan_i32", 257, 1000, seed=3, distinct_in=16)
    assert R.refine_reference(many)[1] > 33153 // 3


def test_the_old_partition_is_reproduced_where_nothing_splits():
    for kind, kw in (("proj", dict(r=4)), ("chan_i32", dict(T=8)), ("chan_f32", dict(T=1)), ("joint", dict(r=1, T=2))):
        case = R.make_case(kind, 23, subs=1, seed=11, classes=12, **kw)
        lab, nparts, _ = R.refine_reference(case)
        assert np.array_equal(lab, R.old_labels(case).astype(np.uint32)) and nparts == int(lab.max())


def test_every_component_of_the_key_splits_some_class():
    """A kernel that drops one channel, or the rounded projection, from a signature cannot reproduce the reference's labels of the
    generic cases: without that column of the key tuples some classes merge."""
    for kind, kw in (("proj", dict(r=1)), ("proj", dict(r=4)), ("chan_i32", dict(T=1)), ("chan_i32", dict(T=8)), ("chan_f32", dict(T=4)),
                     ("joint", dict(r=1, T=2)), ("joint", dict(r=4, T=4))):
        for n in (57, 257):
            case = R.make_case(kind, n, seed=1000 * n, **kw)
            cols, zero = R.key_columns(case)
            full = len(np.unique(np.stack(cols, axis=1), axis=0))
            assert full == R.canonical(cols, zero)[1] + 1
            for drop in range(1, len(cols)):
                rest = cols[:drop] + cols[drop + 1:]
                fewer = len(np.unique(np.stack(rest, axis=1), axis=0)) if rest else 1
                assert fewer < full, (kind, kw, n, drop)


def test_channel_extremes_are_at_entries_the_kernels_read():
    """int32 channels over the full range: INT32_MIN, INT32_MIN + 1 and INT32_MAX (float channels: +-(2^24 - 1)) sit at entries of the
    source, not only in the table or in the noise, in every layout and also where nothing splits (the needles' base case)."""
    for kind, T, r in (("chan_i32", 1, 0), ("chan_i32", 2, 0), ("chan_i32", 8, 0), ("joint", 2, 1), ("joint", 4, 4), ("chan_f32", 1, 0), ("chan_f32", 4, 0)):
        want = R.CHAN_EXTREMES[np.float32 if kind == "chan_f32" else np.int32]
        for n, packed, lab_packed, subs in ((5, 1, 1, 3), (57, 1, 1, 3), (57, 1, 0, 3), (57, 0, 0, 3), (257, 1, 1, 3), (57, 1, 1, 1)):
            if kind == "joint" and not packed:
                continue
            case = R.make_case(kind, n, T=T, r=r, packed=packed, lab_packed=lab_packed, seed=n + T, classes=34 if n > 5 else 4, subs=subs)
            ii, jj = R.entries(n, packed)
            ld = case["ld"]
            read = np.concatenate([case["C"][t * ld * ld + jj * ld + ii] for t in range(T)]).astype(np.int64)
            for v in want:
                assert (read == v).any(), (kind, T, n, packed, lab_packed, subs, v)


def test_planted_values_fall_where_the_header_says():
    for mode in ("nearest", "trunc"):
        case = R.make_planted_case("proj", 57, mode, seed=5)
        sc = R.round_scale(R.ATOL, mode)
        assert sc == (1e7 if mode == "nearest" else -1e7)
        y, l = R.projected(case), R.old_labels(case)
        code = R.round_key(y, R.ATOL, sc)
        for target in R.PLANTS:
            for lab in (0, R.TINY_LABEL):
                assert int(((y == target) & (l == lab)).sum()) == 2, (target, lab)
        assert (code[y == R.ATOL] != 0).all() and (code[y == np.nextafter(R.ATOL, 0.0)] == 0).all()
        k = lambda v: int(R.round_key(np.array([v]), R.ATOL, sc)[0])  # noqa: E731
        # 0.25 - 2^-32: the mantissa 0.99999999907 rounds to 1.0 and folds onto 0.25; truncation keeps 9999999
        assert (k(0.25 - 2.0 ** -32) == k(0.25)) == (mode == "nearest")
        assert (k(0.0625 - 2.0 ** -40) == k(0.0625)) == (mode == "nearest")
        assert k(-(0.25 - 2.0 ** -32)) != k(0.25 - 2.0 ** -32)
        lab_new, _, _ = R.refine_reference(case)
        zero_class = (l == 0) & (np.abs(y) < R.ATOL)
        assert np.array_equal(lab_new == 0, zero_class)
        below = (y == np.nextafter(R.ATOL, 0.0)) & (l == R.TINY_LABEL)
        assert (lab_new[below] != 0).all() and len(set(lab_new[below])) == 1


def test_fmix_inverse_and_key_with_uniform():
    z = np.array([0, 1, 0xDEADBEEF, R.M64, 0x0123456789ABCDEF], dtype=np.uint64)
    for v, f in zip(z, R.fmix64(z)):
        assert R.fmix64_inverse(int(f)) == int(v)
    key, m = R.planted_key()
    assert R.class_uniform(key, np.array([R.TINY_LABEL]))[0] == m * 2.0 ** -53 and m < 2 ** 26


def _header_inputs():
    """A few thousand doubles for both rounding modes: generic ones, values at atol and one ulp around it, mantissas that round up to 1.0,
    negatives, exact ties of the scaled mantissa and their neighbours, zeros, subnormals."""
    rng = np.random.default_rng(99)
    m = 0.5 + 0.5 * rng.random(3000)
    v = np.ldexp(m, rng.integers(-40, 20, size=3000)) * rng.choice([-1.0, 1.0], size=3000)
    ties = (rng.integers(5_000_000, 10_000_000, size=400) + 0.5) / 1e7  # k + 1/2 over the scale: exact where representable
    ties = np.ldexp(ties, rng.integers(-30, 5, size=400))
    near_one = np.ldexp(1.0 - rng.integers(1, 2000, size=300) * 2.0 ** -33, rng.integers(-30, 5, size=300))
    edge = np.array([R.ATOL, np.nextafter(R.ATOL, 0.0), np.nextafter(R.ATOL, 1.0), -R.ATOL, -np.nextafter(R.ATOL, 0.0), 0.0, -0.0, 5e-324, 1e-310,
                     0.0625, np.nextafter(0.0625, 0.0), 0.5, 1.0, np.nextafter(1.0, 0.0), 0.9999999, 0.99999995, 0.99999994999, 1e300, -1e-300])
    return np.concatenate([v, ties, np.nextafter(ties, 0.0), np.nextafter(ties, 9.0), -ties, near_one, -near_one, edge, np.array(R.PLANTS)])


def test_round_key_and_class_uniform_ports_match_the_header():
    vals = _header_inputs()
    assert len(vals) > 5000
    src = r'''
    #include <stdio.h>
    #include <string.h>
    #include "sdpsr_hash.h"
    int main(int argc, char** argv){
      double atol, sc; unsigned long long key; if (scanf("%lf %lf %llu", &atol, &sc, &key) != 3) return 1;
      for (unsigned l = 0; l < 64; ++l) { double u = sdpsr_class_uniform(key, l); unsigned long long b; memcpy(&b, &u, 8); printf("%llu\n", b); }
      unsigned long long bits;
      while (scanf("%llu", &bits) == 1) { double a; memcpy(&a, &bits, 8); printf("%llu\n", (unsigned long long)sdpsr_round_key(a, atol, sc)); }
      return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.check_call(["g++", "-O2", "-I", os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc"), os.path.join(d, "t.cpp"), "-o",
                               os.path.join(d, "t")])
        for atol, mode in ((R.ATOL, "nearest"), (R.ATOL, "trunc"), (1e-3, "nearest"), (1e-12, "trunc")):
            sc = R.round_scale(atol, mode)
            key = R.planted_key()[0] if mode == "trunc" else R.KEY
            text = f"{atol!r} {sc!r} {key}\n" + "\n".join(str(int(b)) for b in vals.view(np.uint64)) + "\n"
            out = subprocess.run([os.path.join(d, "t")], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
            got = np.array([int(w) for w in out], dtype=np.uint64)
            assert len(got) == 64 + len(vals)
            uni = R.class_uniform(key, np.arange(64))  # (label 0 carries no value in the port; the kernels never draw it)
            assert np.array_equal(got[1:64], uni[1:].view(np.uint64))
            want = R.round_key(vals, atol, sc)
            bad = np.flatnonzero(got[64:] != want)
            assert len(bad) == 0, (mode, atol, vals[bad[:5]], got[64:][bad[:5]], want[bad[:5]])


def test_margin_contract_is_what_the_generator_asserts():
    sc = R.round_scale(R.ATOL)
    ok = R._margins_ok(np.array([0.61234565, 0.6123456, R.ATOL * 1.005, R.ATOL * 1.5, 0.0]), R.ATOL, sc)
    assert list(ok) == [False, True, False, True, True]
    ok = R._margins_ok(np.array([0.6123456, 0.61234565]), R.ATOL, -sc)
    assert list(ok) == [False, True]
    with pytest.raises(AssertionError):
        R.check_exact_projection(np.array([0.1]), np.array([0.5]))
