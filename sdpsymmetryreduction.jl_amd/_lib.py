"""ctypes binding of libsdpsr_hip.so (C ABI: include/sdpsr.h).  The library is the
product; this file only declares argument types.  There is no CPU fallback: if the
shared object is missing the import of the binding fails loudly."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdpsr_hip.so")
PROF_LIB_PATH = os.path.join(_HERE, "libsdpsr_prof.so")  # measurement entry points, not the product
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdpsr.h")
PROF_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdpsr_prof.h")

MEM_HOST, MEM_DEVICE = 0, 1
SQUARE_AUTO, SQUARE_I8, SQUARE_F32, SQUARE_F64 = 0, 1, 2, 3
T_TOTAL, T_PROJECT, T_SQUARE, T_REFINE, T_EIGEN, T_ISO, T_IRRED, T_IMAGE, T_COUNT = range(9)
ROUND_NEAREST, ROUND_TRUNC = 0, 1
SETUP_NO_CONSTRAINTS, SETUP_CHOLESKY_QR2, SETUP_MGS = 0, 1, 2  # sdpsr_setup_path
# sdpsr_opts.flags
FLAG_SEPARATE_REFINEMENTS = 1 << 0
FLAG_FRESH_IRREDUCIBLE_ELEMENT = 1 << 1
FLAG_ALWAYS_REORTHOGONALIZE = 1 << 2
FLAG_REFINE_NO_FUSE = 1 << 3
FLAG_UNPACK_EVERY_STEP = 1 << 4
FLAG_SPMM_ONE_BY_ONE = 1 << 5
FLAG_SINGLE_COUPLING_ELEMENT = 1 << 6
FLAG_SMALL_EIGEN_ON_DEVICE = 1 << 7
FLAG_NO_GRAPH = 1 << 8
FLAG_NO_VERIFY_SHORTCUT = 1 << 9
FLAG_FULL_BASIS_IMAGE = 1 << 10
FLAG_ALWAYS_PROJECT = 1 << 11
FLAG_SYTRD_PANELS = 1 << 12
FLAG_COUPLING_ON_HOST = 1 << 13
FLAG_SYTRD_ONE_LAUNCH = 1 << 14
FLAG_WAIT_FOR_EVERY_VERDICT = 1 << 15
FLAG_WIDE_LOOP_LABELS = 1 << 16
FLAG_MODULE_SCRATCH_FILLS = 1 << 17
FLAG_SQUARE_EVERY_VERDICT = 1 << 18
FLAG_CHECKS_IN_LOOP = 1 << 19
FLAG_LABELS_BEFORE_BLOCKDIAG = 1 << 20
BASIS_IMAGE_KERNELS = {"auto": 0, "two_stage": 1, "outer": 2, "chunk": 3}
# sdpsr_basis_image: *route
BI_ROUTE_COMMUTATIVE, BI_ROUTE_BLOCKS, BI_ROUTE_TWO_STAGE, BI_ROUTE_OUTER, BI_ROUTE_CHUNK = 1, 2, 3, 4, 5
BI_ROUTE_REPAIRED, BI_ROUTE_SHORTCUT_REFUSED = 0x100, 0x200
TRI_UPPER, TRI_FULL = 0, 1  # sdpsr_block_images_sparse: triangle
REFINE_PATHS = {"auto": 0, "hash": 1, "sort": 2, "bucket": 3, "no_mid": 4, "mid_no_first": 6}

# sdpsr_set_label_width: the element type of a label array at each interface width (the reference's Partition{T})
LABEL_DTYPES = {8: np.dtype(np.uint8), 16: np.dtype(np.uint16), 32: np.dtype(np.uint32)}


def label_dtype(bits):
    """numpy dtype of a label array at interface width ``bits`` (8, 16 or 32)."""
    try:
        return LABEL_DTYPES[int(bits)]
    except KeyError:
        raise ValueError(f"label width must be 8, 16 or 32, not {bits!r}") from None


STATUS = {
    0: "OK", 1: "INVALID_DECOMPOSITION_FIELD", 2: "NUMERICAL_INCONSISTENCY", 3: "DIMENSION_MISMATCH",
    4: "LABEL_OVERFLOW", 5: "BAD_ARGUMENT", 6: "HIP_ERROR", 7: "SOLVER_ERROR", 8: "OUT_OF_MEMORY",
    9: "NOT_CONVERGED", 10: "BAD_STATE",
}


class Opts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("square_mode", C.c_int32),
        ("channels", C.c_int32),
        ("max_iters", C.c_int32),
        ("confirm_rounds", C.c_int32),
        ("eig_driver", C.c_int32),
        ("flags", C.c_uint32),
        ("round_mode", C.c_int32),
        ("basis_image_kernel", C.c_int32),
        ("refine_path", C.c_int32),
        ("label_bits", C.c_int32),
        ("insert_wgs_per_cu", C.c_int32),
        ("square_kernel", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class SdpOpts(C.Structure):
    """sdpsr_sdp_opts: a zero field selects its default (rho 1, eps 1e-9, max_iters 20000, check_every 50, max, x >= 0)."""
    _fields_ = [
        ("rho", C.c_double),
        ("eps", C.c_double),
        ("max_iters", C.c_int32),
        ("check_every", C.c_int32),
        ("adapt_rho", C.c_int32),
        ("sense", C.c_int32),
        ("nonneg", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class SdpInfo(C.Structure):
    """sdpsr_sdp_info: the report of sdpsr_sdp_solve, computed from the returned x."""
    _fields_ = [
        ("objective", C.c_double),
        ("r_primal", C.c_double),
        ("r_dual", C.c_double),
        ("rho", C.c_double),
        ("eq_residual", C.c_double),
        ("min_x", C.c_double),
        ("lambda_min", C.c_double),
        ("iters", C.c_int32),
        ("rho_changes", C.c_int32),
    ]


def declared_symbols(header_path=HEADER_PATH):
    """Every function the header declares (used by the symbol-export test)."""
    txt = open(header_path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sdpsr_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C sdpsymmetryreduction.jl_amd/csrc` "
            "(there is no CPU fallback for the HIP path)")
    # One HIP runtime per process.  The library asks for `libamdhip64.so.7`; torch's wheels carry their own copy with that
    # SONAME and load it under the file name `libamdhip64.so`.  torch first: the loader hands the library torch's copy (the
    # SONAMEs match) and device pointers, streams and events are shared.  The library first: /opt/rocm's runtime is loaded,
    # a later `import torch` loads its own copy beside it, and that second runtime finds no GPU ("No HIP GPUs are
    # available", tools/gpu/torch_after_lib.py).  So torch, where installed, is imported before the library is opened.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    pi64, pi32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    sigs = {
        "sdpsr_create": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(Opts), C.POINTER(vp)]),
        "sdpsr_destroy": (None, [vp]),
        "sdpsr_last_error": (C.c_char_p, [vp]),
        "sdpsr_status_string": (C.c_char_p, [C.c_int]),
        "sdpsr_version": (C.c_int, []),
        "sdpsr_set_stream": (C.c_int, [vp, vp]),
        "sdpsr_synchronize": (C.c_int, [vp]),
        "sdpsr_wait_stream": (C.c_int, [vp, vp]),
        "sdpsr_set_seed": (C.c_int, [vp, C.c_uint64]),
        "sdpsr_dimension_trajectory": (C.c_int, [vp, vp, i32, pi32]),
        "sdpsr_partition_from_f64": (C.c_int, [vp, i64, vp, vp, pi64, C.c_int]),
        "sdpsr_partition_from_u32": (C.c_int, [vp, i64, vp, vp, pi64, C.c_int]),
        "sdpsr_partition_from_u64": (C.c_int, [vp, i64, vp, vp, pi64, C.c_int]),
        "sdpsr_refine": (C.c_int, [vp, i64, vp, pi64, vp, i64, C.c_int]),
        "sdpsr_partition_checksum": (C.c_int, [vp, i64, vp, vp, C.c_int]),
        "sdpsr_fill": (C.c_int, [vp, i64, vp, vp, i64, vp, C.c_int]),
        "sdpsr_randomize": (C.c_int, [vp, i64, vp, vp, C.c_int]),
        "sdpsr_clamp_round": (C.c_int, [vp, i64, vp, dbl, C.c_int]),
        "sdpsr_project_out": (C.c_int, [vp, i64, vp, vp, i64, C.c_int]),
        "sdpsr_square_f64": (C.c_int, [vp, i64, vp, vp, C.c_int]),
        "sdpsr_square_f32": (C.c_int, [vp, i64, vp, vp, C.c_int]),
        "sdpsr_square_i8": (C.c_int, [vp, i64, vp, vp, C.c_int]),
        "sdpsr_square_i8_symmetric": (C.c_int, [vp, i64, i64, vp, vp, C.c_int]),
        "sdpsr_gemm_tn_f64": (C.c_int, [vp, i64, i64, i64, vp, i64, vp, i64, vp, i64, C.c_int]),
        "sdpsr_admissible_subspace": (C.c_int, [vp, i64, vp, vp, vp, i64, dbl, vp, pi64, pi32, vp, C.c_int]),
        "sdpsr_admissible_subspace_dense": (C.c_int, [vp, i64, i64, vp, vp, vp, dbl, vp, pi64, pi32, vp, C.c_int]),
        "sdpsr_admissible_setup_csr": (C.c_int, [vp, i64, i64, vp, vp, vp, C.c_int, vp, vp, dbl, vp, vp, vp, pi64, C.POINTER(C.c_int),
                                                 pi32, C.c_int]),
        "sdpsr_admissible_subspace_csr": (C.c_int, [vp, i64, i64, vp, vp, vp, C.c_int, vp, vp, dbl, vp, pi64, pi32, vp, C.c_int]),
        "sdpsr_jordan_reduce": (C.c_int, [vp, i64, vp, vp, vp, i64, dbl, dbl, vp, pi64, pi32, pi32, pi64, pi64, vp, i64, vp, i64, vp, C.c_int]),
        "sdpsr_jordan_reduce_batch": (C.c_int, [vp, C.c_int32, vp, i64, vp, vp, vp, i64, dbl, dbl, vp, pi64, pi32, pi32, pi64, pi64, vp, vp, pi32,
                                                C.c_int]),
        "sdpsr_problem_create": (C.c_int, [vp, i64, vp, vp, vp, i64, C.c_int, C.c_int, C.POINTER(vp)]),
        "sdpsr_problem_destroy": (C.c_int, [vp]),
        "sdpsr_problem_reduce": (C.c_int, [vp, vp, dbl, dbl, vp, pi64, pi32, pi32, pi64, pi64, vp, i64, vp, i64, vp, C.c_int]),
        "sdpsr_problem_reduce_batch": (C.c_int, [vp, vp, C.c_int32, vp, dbl, dbl, vp, pi64, pi32, pi32, pi64, pi64, vp, vp, pi32, C.c_int]),
        "sdpsr_batch_block_sizes": (C.c_int, [vp, C.c_int32, vp]),
        "sdpsr_transfer_bytes": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "sdpsr_reduce_constraints": (C.c_int, [vp, i64, vp, i64, i64, vp, vp, C.c_int]),
        "sdpsr_reduce_constraints_csr": (C.c_int, [vp, i64, vp, i64, i64, vp, vp, vp, C.c_int, vp, C.c_int]),
        "sdpsr_sparse_create": (C.c_int, [vp, i64, i64, i64, vp, vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
        "sdpsr_sparse_destroy": (C.c_int, [vp]),
        "sdpsr_sparse_info": (C.c_int, [vp, pi64, pi64, pi64, C.POINTER(C.c_int)]),
        "sdpsr_sparse_export": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_int]),
        "sdpsr_admissible_setup_sparse": (C.c_int, [vp, i64, vp, vp, vp, dbl, vp, vp, vp, pi64, C.POINTER(C.c_int), pi32, C.c_int]),
        "sdpsr_admissible_subspace_sparse": (C.c_int, [vp, i64, vp, vp, vp, dbl, vp, pi64, pi32, vp, C.c_int]),
        "sdpsr_reduce_constraints_sparse": (C.c_int, [vp, vp, vp, i64, vp, C.c_int]),
        "sdpsr_compress_constraints": (C.c_int, [vp, i64, i64, vp, vp, dbl, dbl, vp, pi64, vp, pi64, pi32, C.c_int]),
        "sdpsr_desymmetrize": (C.c_int, [vp, i64, vp, pi64, pi32, C.c_int]),
        "sdpsr_block_diagonalize": (C.c_int, [vp, i64, vp, i64, dbl, pi32, pi64, pi64, vp, C.c_int]),
        "sdpsr_block_sizes": (C.c_int, [vp, vp]),
        "sdpsr_q_hat": (C.c_int, [vp, vp, C.c_int]),
        "sdpsr_block_images": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "sdpsr_basis_image": (C.c_int, [vp, i64, vp, i64, i32, vp, vp, i64, i64, dbl, vp, pi32, vp, C.c_int]),
        "sdpsr_eigen_decomposition": (C.c_int, [vp, i64, vp, i64, dbl, pi32, pi32, C.c_int]),
        "sdpsr_block_diagonalize_complex": (C.c_int, [vp, i64, vp, i64, dbl, vp, pi64, pi32, pi64, pi64, C.c_int]),
        "sdpsr_block_sizes_complex": (C.c_int, [vp, vp]),
        "sdpsr_block_images_complex": (C.c_int, [vp, vp, vp, C.c_int]),
        "sdpsr_basis_image_complex": (C.c_int, [vp, i64, vp, i64, i32, vp, vp, i64, i64, dbl, vp, pi32, vp, C.c_int]),
        "sdpsr_block_images_sparse": (C.c_int, [vp, i32, vp, i64, vp, C.c_int, C.c_int, dbl, C.c_int, i64, vp, vp, vp, vp, vp, pi64,
                                                C.POINTER(C.c_double), C.c_int]),
        "sdpsr_eigen_decomposition_batched": (C.c_int, [vp, i64, vp, i64, dbl, i64, vp, vp, vp, vp, C.c_int]),
        "sdpsr_syev_f64": (C.c_int, [vp, i64, vp, vp, vp, C.c_int]),
        "sdpsr_hint_symmetric_basis": (C.c_int, [vp, C.c_int]),
        "sdpsr_set_label_width": (C.c_int, [vp, C.c_int]),
        "sdpsr_label_width": (C.c_int, [vp]),
        "sdpsr_set_psd_max_order": (C.c_int, [vp, C.c_int]),
        "sdpsr_psd_max_order": (C.c_int, [vp]),
        "sdpsr_labels_convert": (C.c_int, [vp, i64, vp, C.c_int, vp, C.c_int, C.c_int]),
        "sdpsr_meet_keys": (C.c_int, [vp, i32, vp, vp, i64, i64, vp, C.c_int]),
        "sdpsr_agree_partitions": (C.c_int, [vp, vp, i32, vp, vp, i64, pi64, pi32, C.c_int]),
        "sdpsr_agree_block_diagonalization": (C.c_int, [vp, vp, i32, i32, vp, pi32, pi32, vp, i32]),
        "sdpsr_comm_unique_id": (C.c_int, [vp]),
        "sdpsr_comm_create": (C.c_int, [vp, i32, i32, vp, C.POINTER(vp)]),
        "sdpsr_comm_rank": (C.c_int, [vp]),
        "sdpsr_comm_world": (C.c_int, [vp]),
        "sdpsr_comm_broadcast": (C.c_int, [vp, vp, vp, i64, i32, C.c_int]),
        "sdpsr_comm_destroy": (C.c_int, [vp]),
        "sdpsr_blockop_create": (C.c_int, [vp, i32, vp, i64, i64, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "sdpsr_blockop_destroy": (C.c_int, [vp]),
        "sdpsr_blockop_info": (C.c_int, [vp, pi64, pi32, pi64, pi64]),
        "sdpsr_blockop_apply": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "sdpsr_blockop_adjoint": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "sdpsr_blocks_syev": (C.c_int, [vp, i32, vp, vp, vp, vp, C.c_int]),
        "sdpsr_psd_project": (C.c_int, [vp, i32, vp, vp, vp, vp, C.c_int]),
        "sdpsr_sdp_solve": (C.c_int, [vp, vp, i64, vp, vp, vp, C.POINTER(SdpOpts), vp, vp, vp, C.POINTER(SdpInfo), C.c_int]),
    }
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"libsdpsr_hip.so lacks symbols declared in include/sdpsr.h: {missing}")
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_prof = None


def load_prof_library():
    """libsdpsr_prof.so (include/sdpsr_prof.h): per-kernel timing entry points for bench.py's roofline
    leg and tools/ -- built beside the product library, never needed by the product path."""
    global _prof
    if _prof is not None:
        return _prof
    load_library()  # libsdpsr_prof.so links against libsdpsr_hip.so ($ORIGIN rpath)
    if not os.path.exists(PROF_LIB_PATH):
        raise RuntimeError(f"{PROF_LIB_PATH} is missing: build it with `make -C sdpsymmetryreduction.jl_amd/csrc`")
    lib = C.CDLL(PROF_LIB_PATH)
    vp, i64 = C.c_void_p, C.c_int64
    for name in ("sdpsr_profile_kernel", "sdpsr_profile_clock"):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [vp, C.c_int, i64, i64, C.c_int, C.POINTER(C.c_double)]
    lib.sdpsr_profile_band_chase.restype = C.c_int
    lib.sdpsr_profile_band_chase.argtypes = [vp, i64, C.c_int, vp, vp, vp, C.POINTER(C.c_double)]
    lib.sdpsr_profile_band_reduce.restype = C.c_int
    lib.sdpsr_profile_band_reduce.argtypes = [vp, i64, C.c_int, vp, C.POINTER(C.c_double)]
    lib.sdpsr_profile_host_waits.restype = C.c_int
    lib.sdpsr_profile_host_waits.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_loop_counts.restype = C.c_int
    lib.sdpsr_profile_loop_counts.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_sytrd_graphs.restype = C.c_int
    lib.sdpsr_profile_sytrd_graphs.argtypes = [vp, C.POINTER(C.c_double)]
    lib.sdpsr_profile_gather_packed.restype = C.c_int
    lib.sdpsr_profile_gather_packed.argtypes = [vp, i64, C.c_int, i64, C.c_uint64, vp, vp, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_verify.restype = C.c_int
    lib.sdpsr_profile_verify.argtypes = [vp, i64, C.c_int, i64, C.c_int, vp, vp, vp, vp, C.c_double, C.c_uint64, C.c_double,
                                         C.POINTER(C.c_uint32)]
    lib.sdpsr_profile_basis_constant.restype = C.c_int
    lib.sdpsr_profile_basis_constant.argtypes = [vp, i64, C.c_int, i64, vp, vp, vp, C.c_double, C.POINTER(C.c_uint32)]
    lib.sdpsr_profile_verify_pair.restype = C.c_int
    lib.sdpsr_profile_verify_pair.argtypes = [vp, i64, i64, vp, vp, vp, vp, C.POINTER(C.c_uint32)]
    lib.sdpsr_profile_initial_guess.restype = C.c_int
    lib.sdpsr_profile_initial_guess.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    # the loop's label consumers at either label width (32, or 8: the shadow of the guessed-closed path)
    lib.sdpsr_profile_narrow_labels.restype = C.c_int
    lib.sdpsr_profile_narrow_labels.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_gather_packed_w.restype = C.c_int
    lib.sdpsr_profile_gather_packed_w.argtypes = [vp, i64, C.c_int, i64, C.c_uint64, C.c_int, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_verify_w.restype = C.c_int
    lib.sdpsr_profile_verify_w.argtypes = [vp, i64, C.c_int, i64, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_uint64, C.c_double, C.POINTER(C.c_uint32)]
    lib.sdpsr_profile_verify_pair_w.restype = C.c_int
    lib.sdpsr_profile_verify_pair_w.argtypes = [vp, i64, i64, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_uint32)]
    lib.sdpsr_profile_square_checks.restype = C.c_int
    lib.sdpsr_profile_square_checks.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_deferred_checks.restype = C.c_int
    lib.sdpsr_profile_deferred_checks.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_recorded_labels.restype = C.c_int
    lib.sdpsr_profile_recorded_labels.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_square_check.restype = C.c_int
    lib.sdpsr_profile_square_check.argtypes = [vp, i64, i64, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_proj_coef_lower.restype = C.c_int
    lib.sdpsr_profile_proj_coef_lower.argtypes = [vp, i64, i64, C.c_uint64, C.c_int, vp, vp, vp, vp]
    # the full-matrix channel gathers and the projection's dot products on labels, on caller-made inputs (tests)
    lib.sdpsr_profile_gather_full.restype = C.c_int
    lib.sdpsr_profile_gather_full.argtypes = [vp, C.c_int, i64, C.c_int, C.c_int, i64, C.c_uint64, vp, vp, i64, C.POINTER(C.c_uint64)]
    lib.sdpsr_profile_proj_coef.restype = C.c_int
    lib.sdpsr_profile_proj_coef.argtypes = [vp, C.c_int, i64, i64, i64, C.c_uint64, vp, vp, vp]
    # one refinement over a computed signature source on caller-made inputs (tests)
    lib.sdpsr_profile_refine_source.restype = C.c_int
    lib.sdpsr_profile_refine_source.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double,
                                                vp, vp, vp, vp, vp, vp, vp, i64, i64, C.c_int, vp, C.POINTER(i64), vp, C.POINTER(C.c_int32)]
    # the module-compression kernels on caller-made inputs (tests)
    f64, rep = C.c_double, C.POINTER(C.c_int32)
    lib.sdpsr_profile_gram.restype = C.c_int
    lib.sdpsr_profile_gram.argtypes = [vp, C.c_int, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, i64, rep]
    lib.sdpsr_profile_tall_times_small.restype = C.c_int
    lib.sdpsr_profile_tall_times_small.argtypes = [vp, i64, i64, i64, i64, i64, f64, f64, i64, vp, vp, vp, i64]
    lib.sdpsr_profile_label_product.restype = C.c_int
    lib.sdpsr_profile_label_product.argtypes = [vp, i64, i64, C.c_int, i64, i64, i64, vp, vp, vp, vp, i64, rep]
    lib.sdpsr_profile_label_product_pair.restype = C.c_int
    lib.sdpsr_profile_label_product_pair.argtypes = [vp, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, i64, rep]
    lib.sdpsr_profile_class_sums2.restype = C.c_int
    lib.sdpsr_profile_class_sums2.argtypes = [vp, i64, i64, C.c_uint32, C.c_int, vp, vp, vp, i64, rep]
    lib.sdpsr_profile_class_sums.restype = C.c_int
    lib.sdpsr_profile_class_sums.argtypes = [vp, i64, i64, i64, vp, vp, vp, i64, rep]
    lib.sdpsr_profile_symmetrize.restype = C.c_int
    lib.sdpsr_profile_symmetrize.argtypes = [vp, i64, i64, vp, i64]
    lib.sdpsr_profile_extract_symmetric.restype = C.c_int
    lib.sdpsr_profile_extract_symmetric.argtypes = [vp, i64, i64, i64, vp, vp, i64]
    lib.sdpsr_profile_normalize_columns.restype = C.c_int
    lib.sdpsr_profile_normalize_columns.argtypes = [vp, i64, i64, i64, i64, vp, vp, vp, i64]
    lib.sdpsr_profile_random_vector.restype = C.c_int
    lib.sdpsr_profile_random_vector.argtypes = [vp, i64, C.c_uint64, vp, i64]
    # the module growth's scratch discipline (tests): each runs the form the ctx's flags choose
    lib.sdpsr_profile_poison_scratch.restype = C.c_int
    lib.sdpsr_profile_poison_scratch.argtypes = [vp]
    lib.sdpsr_profile_stacked_in_place.restype = C.c_int
    lib.sdpsr_profile_stacked_in_place.argtypes = [vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, i64, rep]
    lib.sdpsr_profile_lift.restype = C.c_int
    lib.sdpsr_profile_lift.argtypes = [vp, i64, i64, i64, i64, i64, f64, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_seed_vector.restype = C.c_int
    lib.sdpsr_profile_seed_vector.argtypes = [vp, i64, C.c_uint64, vp, vp, vp, i64]
    lib.sdpsr_profile_qrm_current.restype = C.c_int
    lib.sdpsr_profile_qrm_current.argtypes = [vp, rep]
    # the steps of the complex path on caller-made inputs (tests)
    lib.sdpsr_profile_cx_gather_herm.restype = C.c_int
    lib.sdpsr_profile_cx_gather_herm.argtypes = [vp, i64, vp, C.c_uint64, vp, vp, i64]
    lib.sdpsr_profile_cx_heev.restype = C.c_int
    lib.sdpsr_profile_cx_heev.argtypes = [vp, C.c_int, i64, vp, vp, f64, vp, vp, vp, i64, rep]
    lib.sdpsr_profile_cx_block_norms.restype = C.c_int
    lib.sdpsr_profile_cx_block_norms.argtypes = [vp, C.c_int, i64, vp, vp, vp, vp, vp, C.c_int32, vp, i64]
    lib.sdpsr_profile_cx_irreducible.restype = C.c_int
    lib.sdpsr_profile_cx_irreducible.argtypes = [vp, C.c_int, i64, i64, vp, vp, vp, vp, vp, C.c_int32, f64, vp, i64]
    # the steps of the real dense path on caller-made inputs (tests)
    lib.sdpsr_profile_dense_block_norms.restype = C.c_int
    lib.sdpsr_profile_dense_block_norms.argtypes = [vp, C.c_int, i64, i64, vp, vp, vp, C.c_int32, vp, vp, vp, i64]
    lib.sdpsr_profile_dense_cluster_norms.restype = C.c_int
    lib.sdpsr_profile_dense_cluster_norms.argtypes = [vp, i64, i64, vp, vp, vp, f64, vp, vp, vp, i64]
    lib.sdpsr_profile_dense_classes.restype = C.c_int
    lib.sdpsr_profile_dense_classes.argtypes = [vp, C.c_int32, vp, vp, f64, vp, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_dense_irreducible.restype = C.c_int
    lib.sdpsr_profile_dense_irreducible.argtypes = [vp, C.c_int, i64, i64, i64, vp, vp, i64, vp, C.c_int32, vp, i64, i64, rep]
    lib.sdpsr_profile_copy_cols.restype = C.c_int
    lib.sdpsr_profile_copy_cols.argtypes = [vp, i64, i64, vp, vp, vp, i64, i64, vp, i64, i64, i64]
    lib.sdpsr_profile_clamptol.restype = C.c_int
    lib.sdpsr_profile_clamptol.argtypes = [vp, i64, vp, f64, i64]
    # the stages of the dense symmetric eigensolver on caller-made inputs (tests)
    lib.sdpsr_profile_sytrd.restype = C.c_int
    lib.sdpsr_profile_sytrd.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_backtransform.restype = C.c_int
    lib.sdpsr_profile_backtransform.argtypes = [vp, i64, i64, vp, vp, vp, i64]
    lib.sdpsr_profile_stedc.restype = C.c_int
    lib.sdpsr_profile_stedc.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64]
    # the row-space kernels of compress_constraints on caller-made inputs (tests)
    lib.sdpsr_profile_rowspace_scale.restype = C.c_int
    lib.sdpsr_profile_rowspace_scale.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64]
    lib.sdpsr_profile_rowspace_gram.restype = C.c_int
    lib.sdpsr_profile_rowspace_gram.argtypes = [vp, i64, i64, vp, vp, i64, rep]
    lib.sdpsr_profile_rowspace_rotate.restype = C.c_int
    lib.sdpsr_profile_rowspace_rotate.argtypes = [vp, i64, i64, vp, vp, i64, rep]
    lib.sdpsr_profile_rowspace_finish.restype = C.c_int
    lib.sdpsr_profile_rowspace_finish.argtypes = [vp, i64, i64, i64, vp, vp, f64, C.c_int, vp, vp, vp, C.POINTER(i64), i64]
    _prof = lib
    return lib
