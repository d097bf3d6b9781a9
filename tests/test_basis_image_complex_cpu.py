"""The host side of sdpsr_basis_image_complex: the declaration and its ctypes signature, the wrapper's handling of a
complex Q_hat, the closed form the GPU tests use, and the premise of their bound (tests/test_gpu_basis_image_complex.py)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import basis_image_complex_helpers as H

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_header_declares_the_entry_and_lib_carries_its_signature(pkg):
    text = (ROOT / "include" / "sdpsr.h").read_text()
    m = re.search(r"int\s+sdpsr_basis_image_complex\s*\(([^;]*)\)\s*;", text)
    assert m, "include/sdpsr.h does not declare sdpsr_basis_image_complex"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["sdpsr_ctx* ctx", "int64_t n", "const uint32_t* P", "int64_t d", "int32_t nblocks", "const int32_t* blk_sizes",
                    "const double* Q_hat", "int64_t class_first", "int64_t class_count", "double atol", "double* blks",
                    "int32_t* route", "double* phase_ms", "int mem"]
    src = (ROOT / "sdpsymmetryreduction.jl_amd" / "_lib.py").read_text()
    sig = re.search(r'"sdpsr_basis_image_complex":\s*\(C\.c_int,\s*\[([^\]]*)\]\)', src)
    real = re.search(r'"sdpsr_basis_image":\s*\(C\.c_int,\s*\[([^\]]*)\]\)', src)
    assert sig and real and sig.group(1).split() == real.group(1).split()  # the same fourteen arguments as the real entry
    assert len(sig.group(1).split(",")) == 14
    assert "src/diagonalize.jl:64-89" in text[m.start() - 6000:m.start()] and "src/compat.jl:54-57" in text[m.start() - 6000:m.start()]


def test_q_hat_arg_keeps_a_complex_dtype(pkg):
    n = 6
    rng = np.random.default_rng(1)
    zs = [rng.standard_normal((n, s)) + 1j * rng.standard_normal((n, s)) for s in (2, 1)]
    M, sizes = pkg.api._q_hat_arg(zs, n)
    assert M.dtype == np.complex128 and sizes == [2, 1]
    assert np.array_equal(M, np.concatenate(zs, axis=1))  # the imaginary parts are still there
    M, sizes = pkg.api._q_hat_arg([z.astype(np.complex64) for z in zs], n)
    assert M.dtype == np.complex128
    M, sizes = pkg.api._q_hat_arg([zs[0], zs[1].real], n)  # one complex block makes the matrix complex
    assert M.dtype == np.complex128 and np.array_equal(M[:, 2:], zs[1].real)
    M, sizes = pkg.api._q_hat_arg((np.concatenate(zs, axis=1), [2, 1]), n)
    assert np.iscomplexobj(M)
    for real in ([z.real for z in zs], [z.real.astype(np.float32) for z in zs], [np.ones((n, 2), dtype=np.int64), np.ones((n, 1), dtype=np.int64)]):
        M, sizes = pkg.api._q_hat_arg(real, n)
        assert M.dtype == np.float64 and sizes == [2, 1]
    torch = pytest.importorskip("torch")
    M, _ = pkg.api._q_hat_arg([torch.from_numpy(z) for z in zs], n)
    assert M.dtype == torch.complex128 and pkg.api._is_complex(M)
    M, _ = pkg.api._q_hat_arg([torch.from_numpy(z.real.copy()) for z in zs], n)
    assert M.dtype == torch.float64 and not pkg.api._is_complex(M)


class _NoLibrary:
    """A context whose library must not be reached: the wrapper has to refuse before it."""
    label_width = 32
    label_dtype = np.dtype(np.uint32)

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper went on to the library ({name})")


def test_wrapper_checks_a_complex_q_hat_before_the_library(pkg):
    L, d = H.instance("Z16K5")
    n = L.shape[0]
    P = pkg.Partition(d, L.astype(np.uint32))
    z = np.zeros((n, 3), dtype=np.complex128)
    with pytest.raises(ValueError, match="rows"):
        pkg.basis_image([z[:-1]], P, ctx=_NoLibrary())
    with pytest.raises(ValueError, match="sum to"):
        pkg.basis_image((z, [2, 2]), P, ctx=_NoLibrary())
    for classes in [(0, 1), (d, 2), (1, -1)]:
        with pytest.raises(ValueError, match="window"):
            pkg.basis_image([z], P, classes=classes, ctx=_NoLibrary())


@pytest.mark.parametrize("m", [1, 3, 63])
def test_closed_form_on_the_cyclic_group(m):
    """directed(m) with Q_k = k-th Fourier column / sqrt(m), all blocks 1 x 1: blks[1 + t][k] = omega^(t k)."""
    ref = H.reference_images_complex(H.directed(m), m, H.fourier_columns(m), (1,) * m)
    want = H.fourier_closed_form(m)
    assert ref.shape == want.shape == (m, m)
    assert float(np.abs(ref - want).max()) <= 1e-14  # fp64 exp and sqrt on the way in; the sums are clongdouble
    if m == 3:  # C_3 as the reference writes it (test/runtests.jl:50-54) is the transpose: omega^(-t k)
        assert np.array_equal(H.C3, H.directed(3).T)
        ref3 = H.reference_images_complex(H.C3, 3, H.fourier_columns(3), (1, 1, 1))
        assert float(np.abs(ref3 - H.fourier_closed_form(3, -1)).max()) <= 1e-14


@pytest.mark.parametrize("name", sorted(H.GAUSSIAN_SIZES))
def test_fp64_evaluation_is_far_inside_the_bound(name):
    """The GPU tests hold the library to 2e-12 n against the clongdouble formula.  That presumes fp64 rounding of the same
    sums is negligible: the plain complex128 evaluation must stay within a tenth of the bound for the very Q the GPU tests
    use (the rule of tests/test_basis_image_window_cpu.py).  And no non-zero image may lie anywhere near atol = 1e-12 n,
    where the two sides could clamp differently."""
    L, d = H.instance(name)
    n = L.shape[0]
    sizes, Q, ref = H.gaussian_case(name)
    assert np.allclose(np.linalg.norm(Q, axis=0), 1.0, atol=1e-15)
    f64 = H.reference_images_complex(L, d, Q, sizes, dtype=np.complex128)
    err = float(np.abs(f64.astype(np.clongdouble) - ref).max())
    print(f"basis_image_complex fp64 {name} n={n} d={d} err={err:.3e} tenth={0.1 * 2e-12 * n:.3e}")
    assert err <= 0.1 * 2e-12 * n, (err, n)
    mags = np.abs(ref)
    assert float(mags[mags > 0].min()) > 1e-5 > 1e3 * 1e-12 * n
    if not (L == 0).any():  # the classes partition the entries: the images add up to Q_k^H J Q_k = conj(column sums) (column sums)^T
        tot, c0, off = ref.sum(axis=0), 0, 0
        for s in sizes:
            cs = Q[:, c0:c0 + s].sum(axis=0)
            assert np.allclose(np.asarray(tot[off:off + s * s], dtype=np.complex128).reshape(s, s, order="F"), np.outer(cs.conj(), cs), atol=1e-9)
            c0 += s
            off += s * s


def test_instances_are_what_the_gpu_tests_say_they_are():
    for name, (n, d, sym) in {"Z3K70": (210, 6, False), "M4K17": (68, 32, False), "Z16K5": (80, 32, False), "DSF": (76, 319, False),
                              "N1": (1, 1, True), "C3": (3, 3, False), "P4": (4, 3, True)}.items():
        L, dd = H.instance(name)
        assert (L.shape[0], dd, bool((L == L.T).all())) == (n, d, sym), name
        assert L.max() == dd and L.min() >= 0
    cnt = np.bincount(H.instance("Z3K70")[0].ravel())
    assert sorted(set(cnt[1:])) == [210, 14490] and 14490 == 3 * 4096 + 2202
    cnt = np.bincount(H.instance("M4K17")[0].ravel())
    assert sorted(set(cnt[1:])) == [17, 272]
    L, _ = H.instance("DSF")
    assert (L == 0).sum() > L.size // 2
