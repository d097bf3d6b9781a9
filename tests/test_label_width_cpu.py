"""Label arrays in the reference's own widths (Partition{T}, T = UInt8 / UInt16 / UInt32) across the ABI: what can be checked
without a GPU -- the three functions are declared and exported, the ABI version and the opts layout did not move, the binding
maps widths to dtypes, and the NumPy reference the GPU tests compare against is right on the edge values."""
import ctypes as C
import re

import numpy as np
import pytest

import label_width_ref as ref

NEW_FUNCTIONS = ("sdpsr_set_label_width", "sdpsr_label_width", "sdpsr_labels_convert")


def test_header_declares_and_library_exports_the_label_width_functions(pkg):
    L = pkg._lib
    declared = L.declared_symbols()
    lib = pkg.load_library()
    for name in NEW_FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
    hdr = re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"int\s+sdpsr_set_label_width\s*\(\s*sdpsr_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", hdr)
    assert re.search(r"int\s+sdpsr_label_width\s*\(\s*sdpsr_ctx\s*\*\s*\w+\s*\)", hdr)
    assert re.search(r"int\s+sdpsr_labels_convert\s*\(\s*sdpsr_ctx\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)", hdr)
    # the binding gave them argument types (a call with a Python int for len must not truncate it to 32 bits)
    assert lib.sdpsr_labels_convert.argtypes[1] is C.c_int64
    assert lib.sdpsr_set_label_width.restype is C.c_int and lib.sdpsr_label_width.restype is C.c_int


def test_abi_version_and_opts_layout_did_not_move(pkg):
    L = pkg._lib
    assert pkg.load_library().sdpsr_version() == 5
    assert C.sizeof(L.Opts) == 64
    assert L.Opts.label_bits.offset == 40 and L.Opts.reserved.offset == 52  # no reserved word was named for the width


def test_null_ctx_is_a_bad_argument(pkg):
    lib = pkg.load_library()
    assert lib.sdpsr_set_label_width(None, 16) == 5
    assert lib.sdpsr_label_width(None) == 5
    assert lib.sdpsr_labels_convert(None, 1, None, 32, None, 16, 0) == 5


def test_binding_maps_widths_to_dtypes(pkg):
    L = pkg._lib
    assert L.label_dtype(8) == np.uint8 and L.label_dtype(16) == np.uint16 and L.label_dtype(32) == np.uint32
    assert {b: L.LABEL_DTYPES[b].itemsize * 8 for b in (8, 16, 32)} == {8: 8, 16: 16, 32: 32}
    for bad in (0, 12, 64):
        with pytest.raises(ValueError):
            L.label_dtype(bad)
    assert callable(pkg.labels_convert)


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_reference_conversion_on_edge_values(bits):
    edge = np.array([0, 255, 256, 65535, 65536], dtype=np.uint32)
    fits = edge[edge <= ref.typemax(bits)]
    out = ref.convert_reference(fits, bits)
    assert out.dtype == ref.DTYPES[bits] and np.array_equal(out.astype(np.uint64), fits.astype(np.uint64))
    for v in edge[edge > ref.typemax(bits)]:
        with pytest.raises(ref.Inexact):
            ref.convert_reference(np.array([0, v, 1], dtype=np.uint32), bits)
    # exactly typemax fits, typemax + 1 does not (8 and 16 bits)
    assert ref.convert_reference(np.array([ref.typemax(bits)], dtype=np.uint64), bits)[0] == ref.typemax(bits)
    if bits < 32:
        with pytest.raises(ref.Inexact):
            ref.convert_reference(np.array([ref.typemax(bits) + 1], dtype=np.uint32), bits)
    # widening back is the identity
    assert np.array_equal(ref.convert_reference(out, 32), fits)


@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("len_", [1, 7, 17, 4097])
def test_random_labels_carry_the_edge_values(bits, len_):
    a = ref.random_labels(len_, bits, seed=len_)
    assert a.size == len_ and int(a.max()) == ref.typemax(bits)
    assert a[0] == ref.typemax(bits)
    if len_ >= 3:
        assert a[len_ - 1] == ref.typemax(bits) and a[len_ // 2] == 0
