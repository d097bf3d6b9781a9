"""sdpsr-hip: MI355X-native Jordan-reduction path of SDPSymmetryReduction.jl.

The directory name is not an importable dotted name; load it with
``__graft_entry__.load_package()`` (imports it as ``sdpsr_amd``).
"""
from . import parallel  # noqa: F401
from . import _lib  # noqa: F401
from . import api  # noqa: F401
from ._lib import (MEM_DEVICE, MEM_HOST, SQUARE_AUTO, SQUARE_F32, SQUARE_F64, SQUARE_I8,  # noqa: F401
                   load_library)
from .api import (BlockDiagonalization, Context, DimensionMismatch, InvalidDecompositionField,  # noqa: F401
                  LabelOverflow, NotConverged, NumericalInconsistency, Partition, SdpsrError,
                  admissible_setup, admissible_setup_csr, admissible_subspace, basis_image, class_window, csr_arrays, blockDiagonalize, default_context, desymmetrize, unSymmetrize,
                  diagonalize, dim, eigen_decomposition, jordan_reduce_batch, Problem, eigen_decomposition_batched, fill, labels_convert, partition_checksum, randomize, reduce_constraints,
                  reduce_constraints_csr, SparseConstraints, compress_constraints, reduced_sdp,
                  refine, relabel_keys, SparseBlocks, basis_image_sparse, block_images_sparse,
                  BlockOperator, block_eigvals, block_spectrum_check, psd_project, reduce_and_solve, SolveResult)
from . import agree  # noqa: F401
from .agree import Comm, agree_block_diagonalization, agree_partitions, meet_keys  # noqa: F401
