# SDPSymmetryReductionHIP.jl -- Julia-side binding of libsdpsr_hip.so (include/sdpsr.h).
#
# WRITTEN BLIND: there is no Julia toolchain in the build image, so this file has never been
# executed.  It shows the binding a maintainer of SDPSymmetryReduction.jl would add: a new
# `AbstractPartition` backend whose whole-function specialisations are one `ccall` each
# (the generic functions call `mul!`/`eigen` on plain matrices, so the backend specialises
# `admissible_subspace(::Type{HIPPartition}, ...)`, `diagonalize(::Type{Float64}, ::HIPPartition)`
# and `basis_image(Q, ::HIPPartition)`, exactly where test/partitions_set.jl plugs in its
# `Partition{BitSet}`).
module SDPSymmetryReductionHIP

import SDPSymmetryReduction as SR
using LinearAlgebra, SparseArrays

const libsdpsr = get(ENV, "SDPSR_HIP_LIB", "libsdpsr_hip.so")
const MEM_HOST = Cint(0)

struct StatusError <: Exception
    code::Cint
    msg::String
end

# sdpsr_opts (include/sdpsr.h, ABI 0.3): 16 32-bit words; everything zero = the library's defaults
struct Opts
    struct_size::UInt32
    square_mode::Int32
    channels::Int32
    max_iters::Int32
    confirm_rounds::Int32
    eig_driver::Int32
    flags::UInt32            # SDPSR_FLAG_*
    round_mode::Int32        # 0 nearest (default), 1 trunc = unsafe_round as written (utils.jl:49-53)
    basis_image_kernel::Int32
    refine_path::Int32
    label_bits::Int32        # 8 * sizeof(T) of Partition{T}: InexactError where the reference throws it; 0 = never
    insert_wgs_per_cu::Int32 # measurement knob, 0 = default
    square_kernel::Int32     # 0 = by size, 1 = 128 x 128 tiles, 64 = persistent 256 x 256 launch forced
    reserved::NTuple{3,Int32}
end
# SDPSR_FLAG_* (A/B switch, same results either way; the full list is in include/sdpsr.h)
const FLAG_CHECKS_IN_LOOP = UInt32(1) << 19   # the guessed-closed path's verdict-only checks run in the loop, not in blockDiagonalize's waits
Opts(; flags=0, round_mode=0, label_bits=0, square_mode=0, channels=0) =
    Opts(UInt32(64), square_mode, channels, 0, 0, 0, UInt32(flags), round_mode, 0, 0, label_bits, 0, 0, (Int32(0), Int32(0), Int32(0)))

mutable struct Context
    handle::Ptr{Cvoid}
    function Context(; device::Integer=0, seed::Integer=rand(UInt64), opts::Opts=Opts())
        h = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:sdpsr_create, libsdpsr), Cint, (Cint, UInt64, Ref{Opts}, Ref{Ptr{Cvoid}}),
                   device, seed % UInt64, Ref(opts), h)
        st == 0 || throw(StatusError(st, "sdpsr_create"))
        ctx = new(h[])
        finalizer(c -> ccall((:sdpsr_destroy, libsdpsr), Cvoid, (Ptr{Cvoid},), c.handle), ctx)
        return ctx
    end
end

const DEFAULT_CTX = Ref{Union{Nothing,Context}}(nothing)
ctx() = (DEFAULT_CTX[] === nothing && (DEFAULT_CTX[] = Context()); DEFAULT_CTX[])

function check(c::Context, st::Cint)
    st == 0 && return
    msg = unsafe_string(ccall((:sdpsr_last_error, libsdpsr), Cstring, (Ptr{Cvoid},), c.handle))
    st == 1 && throw(SR.InvalidDecompositionField(Float64, ComplexF64))   # eigen_decomposition.jl:140
    st == 2 && throw(SR.NumericalInconsistency("eigen_decomposition", msg)) # :152
    st == 3 && throw(DimensionMismatch(msg))                               # diagonalize.jl:6
    st == 4 && throw(InexactError(:refine!, UInt32, 0))                    # partitions.jl:63
    throw(StatusError(st, msg))
end

# ---- the partition backend (AbstractPartition contract, abstract_part.jl:7-16) ----------
# HIPPartition{T} mirrors Partition{T <: Integer} (partitions.jl:6-11) for the label types the library reads and writes as they
# are: T = UInt8, UInt16 (the reference's default in admissible_subspace, partitions.jl:84) or UInt32.  The ctx is told the
# width before every call that passes labels (sdpsr_set_label_width, 8 * sizeof(T)) and P.matrix goes in WITHOUT a widened
# copy; a partition with more than typemax(T) classes is the reference's InexactError (status 4, output untouched).
const LabelT = Union{UInt8,UInt16,UInt32}
mutable struct HIPPartition{T<:LabelT} <: SR.AbstractPartition
    nparts::Int
    matrix::Matrix{T}
end
HIPPartition(nparts::Integer, matrix::Matrix{T}) where {T<:LabelT} = HIPPartition{T}(Int(nparts), matrix)
labeltype(::HIPPartition{T}) where {T} = T
labeltype(::Type{HIPPartition{T}}) where {T} = T
labeltype(::Type{HIPPartition}) = UInt32
function width!(c::Context, ::Type{T}) where {T<:LabelT}
    st = ccall((:sdpsr_set_label_width, libsdpsr), Cint, (Ptr{Cvoid}, Cint), c.handle, 8 * sizeof(T))
    st == 0 || throw(StatusError(st, "sdpsr_set_label_width"))
    return c
end
SR.dim(p::HIPPartition) = p.nparts
Base.size(p::HIPPartition, args...) = size(p.matrix, args...)
Base.:(==)(p::HIPPartition, q::HIPPartition) = p.nparts == q.nparts && p.matrix == q.matrix

HIPPartition(M::AbstractMatrix{<:Real}) = HIPPartition{UInt32}(M)
function HIPPartition{T}(M::AbstractMatrix{<:AbstractFloat}) where {T<:LabelT}   # partitions.jl:24-35
    Md = Matrix{Float64}(M); out = Matrix{T}(undef, size(M)); n = Ref{Int64}(0)
    c = width!(ctx(), T)
    check(c, ccall((:sdpsr_partition_from_f64, libsdpsr), Cint,
                   (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cvoid}, Ref{Int64}, Cint),
                   c.handle, length(Md), Md, out, n, MEM_HOST))
    return HIPPartition(n[], out)
end
function HIPPartition{T}(M::AbstractMatrix{<:Integer}) where {T<:LabelT}         # partitions.jl:37-60
    Mi = Matrix{UInt32}(M); out = Matrix{T}(undef, size(M)); n = Ref{Int64}(0)   # (the entries are keys: they stay UInt32)
    c = width!(ctx(), T)
    check(c, ccall((:sdpsr_partition_from_u32, libsdpsr), Cint,
                   (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Cint),
                   c.handle, length(Mi), Mi, out, n, MEM_HOST))
    return HIPPartition(n[], out)
end
function SR.refine!(p::HIPPartition{T}, q::HIPPartition{T}) where {T}   # partitions.jl:62-66
    d = Ref{Int64}(p.nparts); c = width!(ctx(), T)
    check(c, ccall((:sdpsr_refine, libsdpsr), Cint,
                   (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ref{Int64}, Ptr{Cvoid}, Int64, Cint),
                   c.handle, length(p.matrix), p.matrix, d, q.matrix, q.nparts, MEM_HOST))
    p.nparts = d[]
    return p
end
function Base.fill!(M::AbstractMatrix{Float64}, p::HIPPartition; values::AbstractVector) # :68-75
    @assert length(values) == SR.dim(p)
    v = Vector{Float64}(values); c = width!(ctx(), labeltype(p))
    check(c, ccall((:sdpsr_fill, libsdpsr), Cint,
                   (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Cint),
                   c.handle, length(p.matrix), p.matrix, v, length(v), M, MEM_HOST))
    return M
end
SR._constraints(p::HIPPartition{T}) where {T} = SR._constraints(SR.Partition{T}(p.nparts, p.matrix))

# 128-bit checksum of the canonical labels: a probabilistic `==` (partitions.jl:16-17) that lets
# independent restarts on several GPUs agree without exchanging the n x n label matrices
function checksum(p::HIPPartition)
    out = zeros(UInt64, 2); c = width!(ctx(), labeltype(p))
    check(c, ccall((:sdpsr_partition_checksum, libsdpsr), Cint,
                   (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{UInt64}, Cint),
                   c.handle, length(p.matrix), p.matrix, out, MEM_HOST))
    return (out[1], out[2])
end

# ---- the setup stage (partitions.jl:117-142) of the entries below: C_L, X0_L, U and the hint bits ----
# dense A: qr(A') on the host, as the reference does
function _setup(C::AbstractVector{Float64}, A::AbstractMatrix{Float64}, b::AbstractVector{Float64}, atol)
    n = isqrt(length(C)); @assert n^2 == length(C)
    F = qr(A'); U = Matrix(F.Q)[:, 1:rank(A)]; proj(v) = U * (U' * v)
    c = Vector(C); c .-= proj(c); SR._clamp_round!(c, atol=atol); SR._symmetrize!(c, n)
    x0, _ = SR.Krylov.craig(A, b); SR._symmetrize!(x0, n); x0 = proj(x0); SR._clamp_round!(x0, atol=atol)
    hint = 2 | (all(k -> (M = reshape(view(U, :, k), n, n); isapprox(M, M'; atol=1e-12, rtol=0)), 1:size(U, 2)) ? 1 : 0)
    return n, c, x0, U, hint
end
# sparse A: on the device from CSR (sdpsr_admissible_setup_csr).  The CSC arrays of A' are the CSR arrays of A, so
# sparse(A')'s colptr / rowval / nzval go in unchanged with index_base = 1.  No Q is formed: SPQR's Q of a sparse A'
# lives in SPQR's row permutation, so Matrix(F.Q)[:, 1:rank(A)] is not a basis of rowspace(A) there.  The hint bits
# are the ones the library proved.
function _setup(C::AbstractVector{Float64}, A::SparseMatrixCSC{Float64}, b::AbstractVector{Float64}, atol)
    n = isqrt(length(C)); @assert n^2 == length(C)
    m = size(A, 1); @assert size(A, 2) == n^2 && length(b) == m
    At = sparse(A')
    c = Vector{Float64}(undef, n^2); x0 = Vector{Float64}(undef, n^2); U = Matrix{Float64}(undef, n^2, max(m, 1))
    r = Ref{Int64}(0); hint = Ref{Cint}(0); info = Ref{Int32}(0); cx = ctx()
    check(cx, ccall((:sdpsr_admissible_setup_csr, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Float64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Cint}, Ref{Int32}, Cint),
                    cx.handle, n, m, Vector{Int64}(At.colptr), Vector{Int64}(At.rowval), At.nzval, Cint(1), Vector{Float64}(b),
                    Vector{Float64}(C), atol, c, x0, U, r, hint, info, MEM_HOST))
    return n, c, x0, U[:, 1:r[]], Int(hint[])
end

# ---- admissible_subspace: setup on the host (partitions.jl:117-142; from CSR on the device for a sparse A), loop on
# the device ----
function SR.admissible_subspace(::Type{PT}, C::AbstractVector{T}, A::AbstractMatrix{T},
                                b::AbstractVector{T}; verbose::Bool=false,
                                atol=Base.rtoldefault(real(T))) where {T<:AbstractFloat,PT<:HIPPartition}
    LT = labeltype(PT)   # HIPPartition{UInt16} etc.; plain HIPPartition: UInt32
    n, c, x0, U, hint = _setup(Vector{Float64}(C), A isa SparseMatrixCSC ? SparseMatrixCSC{Float64}(A) : Matrix{Float64}(A),
                               Vector{Float64}(b), atol)
    P = Matrix{LT}(undef, n, n); d = Ref{Int64}(0); it = Ref{Int32}(0); cx = width!(ctx(), LT)
    # symmetric basis matrices (the usual case): the projection step may work on the lower triangle
    # (bit 1: c and x0 were symmetrised)
    ccall((:sdpsr_hint_symmetric_basis, libsdpsr), Cint, (Ptr{Cvoid}, Cint), cx.handle, hint)
    check(cx, ccall((:sdpsr_admissible_subspace, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64,
                     Ptr{Cvoid}, Ref{Int64}, Ref{Int32}, Ptr{Float64}, Cint),
                    cx.handle, n, c, x0, U, size(U, 2), atol, P, d, it, C_NULL, MEM_HOST))
    if verbose  # the reference's log lines (partitions.jl:150,156,187-188) from the dimension trajectory
        cnt = Ref{Int32}(0)
        ccall((:sdpsr_dimension_trajectory, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int32, Ref{Int32}), cx.handle, C_NULL, 0, cnt)
        dims = Vector{Int64}(undef, cnt[])
        ccall((:sdpsr_dimension_trajectory, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int32, Ref{Int32}), cx.handle, dims, cnt[], cnt)
        @info "Starting the reduction. Dimensions:" maximal = (n^2 + n) ÷ 2 initial = dims[1]
        for k in 1:length(dims)-1
            @debug "Iteration $k, Current dimension: $(dims[k])"
        end
        @info "Minimal admissible subspace converged in $(it[]) iterations at dimension:" final = d[]
    end
    return HIPPartition(d[], P)
end

# ---- reduced-SDP assembly from a sparse A (README.md:57-60, test/sd_problems.jl:32-37,113-118):
# newA = reduce_constraints(P, A), newC = reduce_constraints(P, sparse(C')) in place of A * PMat with
# PMat = hcat(vec(P.matrix .== i) for i = 1:dim(P)).  sparse(A')'s colptr / rowval / nzval are the CSR arrays of A and go
# in unchanged with index_base = 1 (sdpsr_reduce_constraints_csr).  WRITTEN BLIND like the rest of this file: never run.
function reduce_constraints(P::HIPPartition, A::SparseMatrixCSC)
    m = size(A, 1); d = Int64(P.nparts); len = length(P.matrix); @assert size(A, 2) == len
    At = sparse(SparseMatrixCSC{Float64}(A)')
    out = Matrix{Float64}(undef, m, d); cx = width!(ctx(), labeltype(P))
    check(cx, ccall((:sdpsr_reduce_constraints_csr, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ptr{Float64}, Cint),
                    cx.handle, len, P.matrix, d, m, Vector{Int64}(At.colptr), Vector{Int64}(At.rowval), At.nzval, Cint(1), out, MEM_HOST))
    return out
end

# ---- a device-resident sparse A (sdpsr_sparse_create): A is validated and canonicalised ONCE, on the device, and both
# consumers -- the setup stage (partitions.jl:117-142, utils.jl:58-66) and A * PMat (README.md:57-60,
# docs/src/examples/ReduceAndSolveJuMP.jl:42-51) -- read the handle where it lies.  sparse(A')'s colptr / rowval / nzval
# are the CSR arrays of A and go in unchanged with index_base = 1; a caller whose arrays are AMDGPU.jl arrays passes
# their device pointers with mem = MEM_DEVICE (SparseConstraints(len, m, rowptr, colind, val; mem=MEM_DEVICE)).
# WRITTEN BLIND like the rest of this file: never run.
mutable struct SparseConstraints
    handle::Ptr{Cvoid}
    len::Int64
    m::Int64
    nnz::Int64            # canonical entries
    rows_symmetric::Bool
    function SparseConstraints(len::Integer, m::Integer, rowptr, colind, val; index_base::Integer=1, mem::Cint=MEM_HOST,
                               nnz::Integer=length(colind))
        cx = ctx(); h = Ref{Ptr{Cvoid}}(C_NULL)
        check(cx, ccall((:sdpsr_sparse_create, libsdpsr), Cint,
                        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Cint, Ref{Ptr{Cvoid}}),
                        cx.handle, len, m, nnz, rowptr, colind, val, Cint(index_base), mem, h))
        ln = Ref{Int64}(0); mm = Ref{Int64}(0); nz = Ref{Int64}(0); sym = Ref{Cint}(0)
        ccall((:sdpsr_sparse_info, libsdpsr), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Cint}), h[], ln, mm, nz, sym)
        s = new(h[], ln[], mm[], nz[], sym[] != 0)
        finalizer(q -> (q.handle != C_NULL && ccall((:sdpsr_sparse_destroy, libsdpsr), Cint, (Ptr{Cvoid},), q.handle); q.handle = C_NULL), s)
        return s
    end
end
function SparseConstraints(A::SparseMatrixCSC)
    At = sparse(SparseMatrixCSC{Float64}(A)')
    return SparseConstraints(size(A, 2), size(A, 1), Vector{Int64}(At.colptr), Vector{Int64}(At.rowval), At.nzval)
end
# the canonical arrays (sdpsr_sparse_export), 1-based by default: sparse(A')'s colptr / rowval / nzval again
function arrays(S::SparseConstraints; index_base::Integer=1)
    rowptr = Vector{Int64}(undef, S.m + 1); colind = Vector{Int64}(undef, S.nnz); val = Vector{Float64}(undef, S.nnz); cx = ctx()
    check(cx, ccall((:sdpsr_sparse_export, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint),
                    cx.handle, S.handle, Cint(index_base), rowptr, colind, val, MEM_HOST))
    return rowptr, colind, val
end
# the setup stage from a handle (sdpsr_admissible_setup_sparse): what _setup returns for a sparse A
function _setup(C::AbstractVector{Float64}, S::SparseConstraints, b::AbstractVector{Float64}, atol)
    n = isqrt(length(C)); @assert n^2 == length(C) == S.len && length(b) == S.m
    c = Vector{Float64}(undef, n^2); x0 = Vector{Float64}(undef, n^2); U = Matrix{Float64}(undef, n^2, max(S.m, 1))
    r = Ref{Int64}(0); hint = Ref{Cint}(0); info = Ref{Int32}(0); cx = ctx()
    check(cx, ccall((:sdpsr_admissible_setup_sparse, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ref{Int64}, Ref{Cint}, Ref{Int32}, Cint),
                    cx.handle, n, S.handle, Vector{Float64}(b), Vector{Float64}(C), atol, c, x0, U, r, hint, info, MEM_HOST))
    return n, c, x0, U[:, 1:r[]], Int(hint[])
end
# setup and loop in one call (sdpsr_admissible_subspace_sparse)
function SR.admissible_subspace(::Type{PT}, C::AbstractVector{T}, S::SparseConstraints, b::AbstractVector{T};
                                atol=Base.rtoldefault(real(T))) where {T<:AbstractFloat,PT<:HIPPartition}
    LT = labeltype(PT); n = isqrt(length(C)); @assert n^2 == length(C) == S.len && length(b) == S.m
    P = Matrix{LT}(undef, n, n); d = Ref{Int64}(0); it = Ref{Int32}(0); cx = width!(ctx(), LT)
    check(cx, ccall((:sdpsr_admissible_subspace_sparse, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Cvoid}, Ref{Int64}, Ref{Int32}, Ptr{Float64}, Cint),
                    cx.handle, n, S.handle, Vector{Float64}(b), Vector{Float64}(C), atol, P, d, it, C_NULL, MEM_HOST))
    return HIPPartition(d[], P)
end
# newA = reduce_constraints(P, S) (sdpsr_reduce_constraints_sparse)
function reduce_constraints(P::HIPPartition, S::SparseConstraints)
    d = Int64(P.nparts); @assert length(P.matrix) == S.len
    out = Matrix{Float64}(undef, S.m, d); cx = width!(ctx(), labeltype(P))
    check(cx, ccall((:sdpsr_reduce_constraints_sparse, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint),
                    cx.handle, S.handle, P.matrix, d, out, MEM_HOST))
    return out
end

# newA2, newB2 = compress_constraints(newA, b) in place of docs/src/examples/ReduceAndSolveJuMP.jl:44-50
#   newConstraints = sparse(svd(Matrix(hcat(A * PMat, b))').U[:, 1:rank(newConstraints)]'); droptol!(newConstraints, 1e-8)
# (sdpsr_compress_constraints): the r independent rows, by descending singular value.  WRITTEN BLIND like the rest of this file: never run.
function compress_constraints(newA::Matrix{Float64}, b::Vector{Float64}; rtol=0.0, droptol=1e-8)
    m, d = size(newA); @assert length(b) == m
    out = Matrix{Float64}(undef, m, d + 1); sv = Vector{Float64}(undef, m); cx = ctx()
    r = Ref{Int64}(0); nnz = Ref{Int64}(0); passes = Ref{Int32}(0)
    check(cx, ccall((:sdpsr_compress_constraints, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ref{Int64}, Ptr{Float64},
                     Ref{Int64}, Ref{Int32}, Cint),
                    cx.handle, m, d, newA, b, Float64(rtol), Float64(droptol), out, r, sv, nnz, passes, MEM_HOST))
    return out[1:r[], 1:d], out[1:r[], d + 1]
end

# ---- the whole reduction in ONE call (sdpsr_jordan_reduce): admissible_subspace + blockDiagonalize with the
# partition staying on the device; the images are fetched with sdpsr_block_images once their size is known ----
function jordan_reduce(C::AbstractVector{Float64}, A::AbstractMatrix{Float64}, b::AbstractVector{Float64};
                       atol=Base.rtoldefault(Float64), epsilon=Base.rtoldefault(Float64), labels::Type{LT}=UInt32) where {LT<:LabelT}
    n, c, x0, U, _ = _setup(C, A, b, atol)
    P = Matrix{LT}(undef, n, n); d = Ref{Int64}(0); it = Ref{Int32}(0); cx = width!(ctx(), LT)
    nb = Ref{Int32}(0); ssq = Ref{Int64}(0); ss = Ref{Int64}(0)
    check(cx, ccall((:sdpsr_jordan_reduce, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Float64, Ptr{Cvoid}, Ref{Int64},
                     Ref{Int32}, Ref{Int32}, Ref{Int64}, Ref{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Cint),
                    cx.handle, n, c, x0, U, size(U, 2), atol, epsilon, P, d, it, nb, ssq, ss, C_NULL, 0, C_NULL, 0, C_NULL, MEM_HOST))
    sizes = Vector{Int32}(undef, nb[])
    check(cx, ccall((:sdpsr_block_sizes, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Int32}), cx.handle, sizes))
    flat = Vector{Float64}(undef, d[] * ssq[])
    check(cx, ccall((:sdpsr_block_images, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                    cx.handle, flat, C_NULL, C_NULL, MEM_HOST))
    return HIPPartition(d[], P), Int.(sizes), reshape(flat, Int(ssq[]), Int(d[]))   # column i = the blocks of class i, concatenated
end

# ---- blockDiagonalize(Float64, P) (compat.jl:46-68) -------------------------------------
function SR.blockDiagonalize(::Type{Float64}, P::HIPPartition, verbose=true;
                             epsilon=Base.rtoldefault(Float64))
    n = size(P, 1); cx = width!(ctx(), labeltype(P))
    nb = Ref{Int32}(0); ssq = Ref{Int64}(0); ss = Ref{Int64}(0)
    check(cx, ccall((:sdpsr_block_diagonalize, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Ref{Int32}, Ref{Int64}, Ref{Int64},
                     Ptr{Float64}, Cint),
                    cx.handle, n, P.matrix, P.nparts, epsilon, nb, ssq, ss, C_NULL, MEM_HOST))
    sizes = Vector{Int32}(undef, nb[])
    check(cx, ccall((:sdpsr_block_sizes, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Int32}), cx.handle, sizes))
    flat = Vector{Float64}(undef, P.nparts * ssq[])
    check(cx, ccall((:sdpsr_block_images, libsdpsr), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                    cx.handle, flat, C_NULL, C_NULL, MEM_HOST))
    blks = Vector{Vector{Matrix{Float64}}}(undef, P.nparts)
    for i in 1:P.nparts
        off = (i - 1) * ssq[]; blks[i] = Matrix{Float64}[]
        for s in sizes
            push!(blks[i], reshape(flat[off+1:off+s*s], Int(s), Int(s))); off += s * s
        end
    end
    return (blkSizes=Int.(sizes), blks=blks)
end

# ---- diagonalize(Float64, P) (diagonalize.jl:25-40): Q_hat itself ---------------------------
function SR.diagonalize(::Type{Float64}, P::HIPPartition; verbose=false, atol=1e-12 * size(P, 1))
    n = size(P, 1); cx = width!(ctx(), labeltype(P))
    nb = Ref{Int32}(0); ssq = Ref{Int64}(0); ss = Ref{Int64}(0)
    st = ccall((:sdpsr_block_diagonalize, libsdpsr), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Ref{Int32}, Ref{Int64}, Ref{Int64}, Ptr{Float64}, Cint),
               cx.handle, n, P.matrix, P.nparts, atol, nb, ssq, ss, C_NULL, MEM_HOST)
    st == 3 || check(cx, st)   # check_block_sizes belongs to blockDiagonalize (compat.jl:60), not to diagonalize
    sizes = Vector{Int32}(undef, nb[])
    check(cx, ccall((:sdpsr_block_sizes, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Int32}), cx.handle, sizes))
    Q = Matrix{Float64}(undef, n, ss[])
    check(cx, ccall((:sdpsr_q_hat, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), cx.handle, Q, MEM_HOST))
    offs = cumsum(vcat(0, Int.(sizes)))
    return [Q[:, offs[k]+1:offs[k+1]] for k in eachindex(sizes)]
end

# ---- basis_image(Q, P; atol) (diagonalize.jl:64-89) of a caller's Q_hat, for a window of classes ----
# Q_hat: the vector of n x s_k matrices diagonalize returns (any real matrices: nothing is assumed about them);
# classes = (first, count), 1-based, e.g. class_window(dim(P), world, rank) after broadcast!(Q_hat, comm; root=winner).
# Returns blks[i][k] for the classes first .. first + count - 1, and with route=true the pair (blks, route).
class_window(d::Integer, parts::Integer, index::Integer) =   # index 0-based; contiguous, sizes within one, empty when parts > d
    (1 + index * div(d, parts) + min(index, rem(d, parts)), div(d, parts) + (index < rem(d, parts) ? 1 : 0))

function basis_image(Q_hat::AbstractVector{<:AbstractMatrix{Float64}}, P::HIPPartition;
                     classes::Tuple{<:Integer,<:Integer}=(1, P.nparts), atol::Real=-1.0, route::Bool=false)
    n = size(P, 1); cx = width!(ctx(), labeltype(P))
    all(q -> size(q, 1) == n, Q_hat) || throw(DimensionMismatch("every block of Q_hat has size(P, 1) rows"))
    sizes = Int32[size(q, 2) for q in Q_hat]
    Q = Matrix{Float64}(reduce(hcat, Q_hat))
    first, count = Int64(classes[1]), Int64(classes[2])
    S = sum(Int64(s)^2 for s in sizes)
    flat = Vector{Float64}(undef, max(count, 0) * S)
    rt = Ref{Int32}(0)
    check(cx, ccall((:sdpsr_basis_image, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{Float64}, Int64, Int64, Float64,
                     Ptr{Float64}, Ref{Int32}, Ptr{Float64}, Cint),
                    cx.handle, n, P.matrix, P.nparts, length(sizes), sizes, Q, first, count, Float64(atol),
                    flat, rt, C_NULL, MEM_HOST))
    blks = Vector{Vector{Matrix{Float64}}}(undef, count)
    for i in 1:count
        off = (i - 1) * S; blks[i] = Matrix{Float64}[]
        for s in sizes
            push!(blks[i], reshape(flat[off+1:off+s*s], Int(s), Int(s))); off += s * s
        end
    end
    return route ? (blks, Int(rt[])) : blks
end

# The same over ComplexF64 (sdpsr_basis_image_complex): blks[i][k] = Q_k' * (P .== i) * Q_k with the adjoint, for a P that need
# not be symmetric -- the desymmetrized partition blockDiagonalize(ComplexF64, P) hands to basis_image (compat.jl:54-57).
# route is SDPSR_BI_ROUTE_OUTER (4) or _CHUNK (5).
function basis_image(Q_hat::AbstractVector{<:AbstractMatrix{ComplexF64}}, P::HIPPartition;
                     classes::Tuple{<:Integer,<:Integer}=(1, P.nparts), atol::Real=-1.0, route::Bool=false)
    n = size(P, 1); cx = width!(ctx(), labeltype(P))
    all(q -> size(q, 1) == n, Q_hat) || throw(DimensionMismatch("every block of Q_hat has size(P, 1) rows"))
    sizes = Int32[size(q, 2) for q in Q_hat]
    Q = Matrix{ComplexF64}(reduce(hcat, Q_hat))         # (re, im) pairs = ComplexF64 layout
    first, count = Int64(classes[1]), Int64(classes[2])
    S = sum(Int64(s)^2 for s in sizes)
    flat = Vector{ComplexF64}(undef, max(count, 0) * S)
    rt = Ref{Int32}(0)
    check(cx, ccall((:sdpsr_basis_image_complex, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{ComplexF64}, Int64, Int64, Float64,
                     Ptr{ComplexF64}, Ref{Int32}, Ptr{Float64}, Cint),
                    cx.handle, n, P.matrix, P.nparts, length(sizes), sizes, Q, first, count, Float64(atol),
                    flat, rt, C_NULL, MEM_HOST))
    blks = Vector{Vector{Matrix{ComplexF64}}}(undef, count)
    for i in 1:count
        off = (i - 1) * S; blks[i] = Matrix{ComplexF64}[]
        for s in sizes
            push!(blks[i], reshape(flat[off+1:off+s*s], Int(s), Int(s))); off += s * s
        end
    end
    return route ? (blks, Int(rt[])) : blks
end

# ---- block images as solver triplets (sdpsr_block_images_sparse; README.md:72-79, ReduceAndSolveJuMP.jl:56-84) ----
# blks: the nested blks[i][k] of basis_image / blockDiagonalize (real, or ComplexF64: taken as the real embedding [re -im; im re]
# of order 2 s_k, ReduceAndSolveJuMP.jl:59-76).  Returns the named tuple (classptr, blk, row, col, val, sizes): the entries of
# class i (1-based) are classptr[i]+1 : classptr[i+1]; blk / row / col are 1-based; sizes are the orders the indices refer to.
# upper=true keeps row <= col only; entries with !(|v| <= tol) are kept, in the order class, block, column-major.
function block_images_sparse(blks::AbstractVector{<:AbstractVector{<:AbstractMatrix{T}}}; upper::Bool=true,
                             tol::Real=0.0) where {T<:Union{Float64,ComplexF64}}
    cx = ctx()
    count = Int64(length(blks))
    sizes = count == 0 ? Int32[1] : Int32[size(b, 1) for b in blks[1]]
    flat = T[]
    for row in blks, b in row
        append!(flat, vec(Matrix{T}(b)))
    end
    isc = T === ComplexF64 ? Cint(1) : Cint(0)
    classptr = Vector{Int64}(undef, count + 1)
    nnz = Ref{Int64}(0)
    sig = (Ptr{Cvoid}, Int32, Ptr{Int32}, Int64, Ptr{Cvoid}, Cint, Cint, Float64, Cint, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32},
           Ptr{Int32}, Ptr{Float64}, Ref{Int64}, Ptr{Float64}, Cint)
    tri = upper ? Cint(0) : Cint(1)   # SDPSR_TRI_UPPER / SDPSR_TRI_FULL
    check(cx, ccall((:sdpsr_block_images_sparse, libsdpsr), Cint, sig, cx.handle, length(sizes), sizes, count, flat, isc, tri,
                    Float64(tol), Cint(1), 0, classptr, C_NULL, C_NULL, C_NULL, C_NULL, nnz, C_NULL, MEM_HOST))   # sizing call
    m = nnz[]
    blk = Vector{Int32}(undef, m); row = Vector{Int32}(undef, m); col = Vector{Int32}(undef, m); val = Vector{Float64}(undef, m)
    m > 0 && check(cx, ccall((:sdpsr_block_images_sparse, libsdpsr), Cint, sig, cx.handle, length(sizes), sizes, count, flat, isc,
                             tri, Float64(tol), Cint(1), m, classptr, blk, row, col, val, nnz, C_NULL, MEM_HOST))
    return (classptr=classptr, blk=blk, row=row, col=col, val=val, sizes=(T === ComplexF64 ? 2 .* sizes : sizes))
end

# ---- the reduced PSD blocks as an operator (sdpsr_blockop_*, sdpsr_blocks_syev): Z_k(x) = sum(blks[i][k] .* x[i] for i = 1:dim(P)),
# ErdosRenyiThetaFunction.jl:83, test/sd_problems.jl:46-52 -- its adjoint and the spectra of all blocks, on the device ----
# sp: what block_images_sparse returns (1-based indices).  The handle is device-resident; close(op) frees it.
mutable struct BlockOperator
    handle::Ptr{Cvoid}
    d::Int64
    sizes::Vector{Int32}
    sum_sq::Int64
    nnz_full::Int64
end
function BlockOperator(sp; upper::Bool=true)
    cx = ctx()
    sizes = Vector{Int32}(sp.sizes); d = Int64(length(sp.classptr) - 1); m = Int64(length(sp.val))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(cx, ccall((:sdpsr_blockop_create, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int32, Ptr{Int32}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Cint, Cint,
                     Cint, Ref{Ptr{Cvoid}}),
                    cx.handle, length(sizes), sizes, d, m, sp.classptr, sp.blk, sp.row, sp.col, sp.val, upper ? Cint(0) : Cint(1), Cint(1),
                    MEM_HOST, h))
    dd = Ref{Int64}(0); nb = Ref{Int32}(0); ssq = Ref{Int64}(0); nf = Ref{Int64}(0)
    ccall((:sdpsr_blockop_info, libsdpsr), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}, Ref{Int64}, Ref{Int64}), h[], dd, nb, ssq, nf)
    op = BlockOperator(h[], dd[], sizes, ssq[], nf[])
    finalizer(close, op)
    return op
end
function Base.close(op::BlockOperator)
    op.handle == C_NULL || ccall((:sdpsr_blockop_destroy, libsdpsr), Cint, (Ptr{Cvoid},), op.handle)
    op.handle = C_NULL
    return nothing
end
function _split_blocks(flat::Vector{Float64}, sizes)
    out = Matrix{Float64}[]; off = 0
    for s in sizes
        push!(out, reshape(flat[off+1:off+s*s], Int(s), Int(s))); off += s * s
    end
    return out
end
# Z(x): the symmetric Z_k as full matrices
function apply(op::BlockOperator, x::AbstractVector{<:Real})
    cx = ctx(); xv = Vector{Float64}(x); Z = Vector{Float64}(undef, op.sum_sq)
    check(cx, ccall((:sdpsr_blockop_apply, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                    cx.handle, op.handle, xv, Z, MEM_HOST))
    return _split_blocks(Z, op.sizes)
end
# g_i = sum_k <blks[i][k], S_k> for symmetric S_k
function adjoint(op::BlockOperator, S::AbstractVector{<:AbstractMatrix{<:Real}})
    cx = ctx(); flat = Float64[]
    for b in S
        append!(flat, vec(Matrix{Float64}(b)))
    end
    g = Vector{Float64}(undef, op.d)
    check(cx, ccall((:sdpsr_blockop_adjoint, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                    cx.handle, op.handle, flat, g, MEM_HOST))
    return g
end
# the spectra of all blocks in one call: (w, V) with w[k] ascending and the eigenvectors as the columns of V[k]
function block_eigen(Z::AbstractVector{<:AbstractMatrix{<:Real}})
    cx = ctx(); sizes = Int32[size(b, 1) for b in Z]; flat = Float64[]
    for b in Z
        append!(flat, vec(Matrix{Float64}(b)))
    end
    w = Vector{Float64}(undef, sum(sizes)); V = Vector{Float64}(undef, length(flat))
    check(cx, ccall((:sdpsr_blocks_syev, libsdpsr), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                    cx.handle, length(sizes), sizes, flat, w, V, MEM_HOST))
    ws = Vector{Float64}[]; off = 0
    for s in sizes
        push!(ws, w[off+1:off+s]); off += s
    end
    return ws, _split_blocks(V, sizes)
end

# ---- solving the reduced SDP (sdpsr_psd_project, sdpsr_sdp_solve): the model of docs/src/examples/ReduceAndSolveJuMP.jl:40-84 by the
# library's first-order (ADMM) solver in CSDP's place -- not an interior-point replacement, see the README ----
# the largest block order psd_project and sdp_solve take through the ctx: 64 (default) or 128 (sdpsr_set_psd_max_order)
function psd_max_order!(order::Integer)
    cx = ctx()
    check(cx, ccall((:sdpsr_set_psd_max_order, libsdpsr), Cint, (Ptr{Cvoid}, Cint), cx.handle, order))
    return psd_max_order()
end
psd_max_order() = Int(ccall((:sdpsr_psd_max_order, libsdpsr), Cint, (Ptr{Cvoid},), ctx().handle))
# P_k = V max(w, 0) V' of every block (orders up to psd_max_order()) and the blocks' smallest eigenvalues
function psd_project(Z::AbstractVector{<:AbstractMatrix{<:Real}})
    cx = ctx(); sizes = Int32[size(b, 1) for b in Z]; flat = Float64[]
    for b in Z
        append!(flat, vec(Matrix{Float64}(b)))
    end
    P = Vector{Float64}(undef, length(flat)); lmin = Vector{Float64}(undef, length(sizes))
    check(cx, ccall((:sdpsr_psd_project, libsdpsr), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                    cx.handle, length(sizes), sizes, flat, P, lmin, MEM_HOST))
    return _split_blocks(P, sizes), lmin
end
struct SdpOpts  # sdpsr_sdp_opts: a zero field selects its default
    rho::Float64; eps::Float64
    max_iters::Int32; check_every::Int32; adapt_rho::Int32; sense::Int32; nonneg::Int32
    reserved::NTuple{5,Int32}
end
struct SdpInfo  # sdpsr_sdp_info
    objective::Float64; r_primal::Float64; r_dual::Float64; rho::Float64; eq_residual::Float64; min_x::Float64; lambda_min::Float64
    iters::Int32; rho_changes::Int32
end
# max / min newC x  s.t.  newA x = newB (independent rows), x >= 0, Z_k(x) PSD.  Returns (x, info, converged); the iteration limit is
# not an error: every output is written as it stands
function solve(op::BlockOperator, newA::AbstractMatrix{<:Real}, newB::AbstractVector{<:Real}, newC::AbstractVector{<:Real};
               sense::Symbol=:max, rho::Real=1.0, eps::Real=1e-9, max_iters::Integer=20000, check_every::Integer=50,
               adapt_rho::Bool=false, nonneg::Bool=true)
    cx = ctx(); A = Matrix{Float64}(newA); b = Vector{Float64}(newB); c = Vector{Float64}(vec(newC))
    opts = Ref(SdpOpts(rho, eps, max_iters, check_every, adapt_rho ? 1 : 0, sense == :max ? 1 : -1, nonneg ? 1 : -1, (0, 0, 0, 0, 0)))
    info = Ref(SdpInfo(0, 0, 0, 0, 0, 0, 0, 0, 0)); x = Vector{Float64}(undef, op.d)
    st = ccall((:sdpsr_sdp_solve, libsdpsr), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{SdpOpts}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ref{SdpInfo}, Cint),
               cx.handle, op.handle, size(A, 1), A, b, c, opts, x, C_NULL, C_NULL, info, MEM_HOST)
    st == 9 || check(cx, st)  # SDPSR_NOT_CONVERGED
    return x, info[], st == 0
end

# ---- blockDiagonalize(ComplexF64, P) (compat.jl:26-32,54-57; n <= 3072 in this library version) ---
function SR.blockDiagonalize(::Type{ComplexF64}, P::HIPPartition, verbose=true;
                             epsilon=Base.rtoldefault(Float64))
    n = size(P, 1); cx = width!(ctx(), labeltype(P))
    Pd = Matrix{labeltype(P)}(undef, n, n); dd = Ref{Int64}(0)
    nb = Ref{Int32}(0); ssq = Ref{Int64}(0); ss = Ref{Int64}(0)
    check(cx, ccall((:sdpsr_block_diagonalize_complex, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Ptr{Cvoid}, Ref{Int64}, Ref{Int32}, Ref{Int64},
                     Ref{Int64}, Cint),
                    cx.handle, n, P.matrix, P.nparts, epsilon, Pd, dd, nb, ssq, ss, MEM_HOST))
    sizes = Vector{Int32}(undef, nb[])
    check(cx, ccall((:sdpsr_block_sizes_complex, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Int32}), cx.handle, sizes))
    flat = Vector{ComplexF64}(undef, dd[] * ssq[])      # (re, im) pairs = ComplexF64 layout
    check(cx, ccall((:sdpsr_block_images_complex, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}, Cint),
                    cx.handle, flat, C_NULL, MEM_HOST))
    blks = Vector{Vector{Matrix{ComplexF64}}}(undef, dd[])
    for i in 1:dd[]
        off = (i - 1) * ssq[]; blks[i] = Matrix{ComplexF64}[]
        for s in sizes
            push!(blks[i], reshape(flat[off+1:off+s*s], Int(s), Int(s))); off += s * s
        end
    end
    return (blkSizes=Int.(sizes), blks=blks)
end

# ---- R independent random restarts of the reduction in ONE call on this task's thread (sdpsr_jordan_reduce_batch):
# the reference's "try again" after NumericalInconsistency / DimensionMismatch (eigen_decomposition.jl:264-270,
# diagonalize.jl:4-9) run side by side; returns the restarts' partitions, statuses and block-size sums, first the sizes
# (images: call jordan_reduce / blockDiagonalize on the partition of the first restart whose status is 0) ----
function jordan_reduce_batch(C::AbstractVector{Float64}, A::AbstractMatrix{Float64}, b::AbstractVector{Float64}, R::Integer;
                             seeds::Union{Nothing,Vector{UInt64}}=nothing, atol=Base.rtoldefault(Float64),
                             epsilon=Base.rtoldefault(Float64), labels::Type{LT}=UInt32) where {LT<:LabelT}
    n, c, x0, U, hint = _setup(C, A, b, atol)
    cx = width!(ctx(), LT)
    Ps = [Matrix{LT}(undef, n, n) for _ in 1:R]
    pP = Ptr{Cvoid}[pointer(P) for P in Ps]
    d = zeros(Int64, R); it = zeros(Int32, R); nb = zeros(Int32, R); ssq = zeros(Int64, R); ss = zeros(Int64, R); st = zeros(Int32, R)
    ccall((:sdpsr_hint_symmetric_basis, libsdpsr), Cint, (Ptr{Cvoid}, Cint), cx.handle, hint)
    GC.@preserve Ps begin
        ccall((:sdpsr_jordan_reduce_batch, libsdpsr), Cint,
              (Ptr{Cvoid}, Int32, Ptr{UInt64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Float64,
               Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64},
               Ptr{Int32}, Cint),
              cx.handle, R, seeds === nothing ? C_NULL : seeds, n, c, x0, U, size(U, 2), atol, epsilon, pP, d, it, nb, ssq, ss,
              C_NULL, C_NULL, st, MEM_HOST)
    end
    return [(status=Int(st[i]), P=HIPPartition(Int(d[i]), Ps[i]), iterations=Int(it[i]), nblocks=Int(nb[i]),
             sum_sq=Int(ssq[i]), sum_s=Int(ss[i])) for i in 1:R]
end
# (the library uploads C_L, X0_L, U once for the R restarts of this call; a caller who makes SEVERAL such calls on one
# problem keeps a `Problem` and calls `reduce_batch(problem, R)`: nothing is uploaded again)

# ---- upload once, restart many (sdpsr_problem_create / sdpsr_problem_reduce_batch): C_L, X0_L, U travel to the device
# ONCE; every later reduce / reduce_batch call names the handle and moves only its results.  `mem` = MEM_DEVICE takes
# device pointers instead (an AMDGPU.jl ROCArray: pass `pointer(a)` of the ROCArray{Float64} -- they are copied on the
# device, the caller's arrays are free on return). ----
const MEM_DEVICE = Cint(1)
mutable struct Problem
    handle::Ptr{Cvoid}
    n::Int
    ctx::Context
    function Problem(C::AbstractVector{Float64}, A::AbstractMatrix{Float64}, b::AbstractVector{Float64};
                     atol=Base.rtoldefault(Float64), cx::Context=ctx())
        n, c, x0, U, hint = _setup(C, A, b, atol)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(cx, ccall((:sdpsr_problem_create, libsdpsr), Cint,
                        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
                        cx.handle, n, c, x0, U, size(U, 2), hint, MEM_HOST, h))
        p = new(h[], n, cx)
        finalizer(q -> (q.handle != C_NULL && ccall((:sdpsr_problem_destroy, libsdpsr), Cint, (Ptr{Cvoid},), q.handle); q.handle = C_NULL), p)
        return p
    end
end

function reduce_batch(p::Problem, R::Integer; seeds::Union{Nothing,Vector{UInt64}}=nothing, atol=Base.rtoldefault(Float64),
                      epsilon=Base.rtoldefault(Float64), labels::Type{LT}=UInt32) where {LT<:LabelT}
    n = p.n; cx = width!(p.ctx, LT)
    Ps = [Matrix{LT}(undef, n, n) for _ in 1:R]
    pP = Ptr{Cvoid}[pointer(P) for P in Ps]
    d = zeros(Int64, R); it = zeros(Int32, R); nb = zeros(Int32, R); ssq = zeros(Int64, R); ss = zeros(Int64, R)
    st = fill(Int32(-1), R)
    rc = GC.@preserve Ps ccall((:sdpsr_problem_reduce_batch, libsdpsr), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{UInt64}, Float64, Float64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32},
               Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int32}, Cint),
              cx.handle, p.handle, R, seeds === nothing ? C_NULL : seeds, atol, epsilon, pP, d, it, nb, ssq, ss, C_NULL, C_NULL, st, MEM_HOST)
    (rc != 0 && all(x -> x <= 0, st)) && check(cx, rc)   # a failure before the restarts started
    return [(status=Int(st[i]), P=HIPPartition(Int(d[i]), Ps[i]), iterations=Int(it[i]), nblocks=Int(nb[i]),
             sum_sq=Int(ssq[i]), sum_s=Int(ss[i])) for i in 1:R]
end

# ---- test/numerical_issues.jl:85-94 in one call: `count` runs of eigen_decomposition on all CUs ----
function eigen_decomposition_batched(P::HIPPartition, count::Integer; atol=1e-12 * size(P, 1))
    n = size(P, 1); cx = width!(ctx(), labeltype(P))
    st = Vector{Int32}(undef, count); ne = similar(st); nc = similar(st)
    check(cx, ccall((:sdpsr_eigen_decomposition_batched, libsdpsr), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32},
                     Ptr{Int32}, Cint),
                    cx.handle, n, P.matrix, P.nparts, atol, count, C_NULL, st, ne, nc, MEM_HOST))
    return (status=st, neig=ne, nclasses=nc)
end

# ---- the agreement of independent restarts (SURVEY 8e): sdpsr_comm_*, sdpsr_agree_partitions,
# sdpsr_agree_block_diagonalization.  One process per GPU; `unique_id()` is made by one rank and distributed by the caller
# (MPI.jl, Distributed, a file).  EVERY RANK MUST MAKE THE SAME SEQUENCE OF COLLECTIVE CALLS; the library adds no time-out. ----
unique_id() = (id = zeros(UInt8, 128);
               st = ccall((:sdpsr_comm_unique_id, libsdpsr), Cint, (Ptr{UInt8},), id);
               st == 0 || throw(StatusError(st, "sdpsr_comm_unique_id (can librccl.so.1 be opened?)")); id)
mutable struct Comm
    handle::Ptr{Cvoid}
    ctx::Context
    function Comm(world::Integer, rank::Integer, id::Vector{UInt8}; cx::Context=ctx())   # collective
        length(id) == 128 || throw(ArgumentError("the unique id has 128 bytes"))
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(cx, ccall((:sdpsr_comm_create, libsdpsr), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ref{Ptr{Cvoid}}),
                        cx.handle, world, rank, id, h))
        return new(h[], cx)   # (no finalizer: the comm goes before its ctx, and destroying it is the caller's collective-free call)
    end
end
Base.close(c::Comm) = (c.handle != C_NULL && ccall((:sdpsr_comm_destroy, libsdpsr), Cint, (Ptr{Cvoid},), c.handle); c.handle = C_NULL; nothing)
comm_rank(c::Comm) = Int(ccall((:sdpsr_comm_rank, libsdpsr), Cint, (Ptr{Cvoid},), c.handle))
comm_world(c::Comm) = Int(ccall((:sdpsr_comm_world, libsdpsr), Cint, (Ptr{Cvoid},), c.handle))
_handle(c::Comm) = c.handle
_handle(::Nothing) = C_NULL
_ctx(c::Comm) = c.ctx
_ctx(::Nothing) = ctx()

# The partitions of this rank's restarts (and, with a comm, of every other rank's) end as ONE partition: when they differ --
# `==`, partitions.jl:16-17, by checksum -- every one of `ps` is overwritten with their meet, refine! (partitions.jl:62-66) folded
# over the valid restarts.  valid[i] = false: restart i holds no partition (its status was not 0, 2 or 3); it is not read and
# receives the result.  Returns true when a meet was needed.  More than typemax(T) classes: InexactError, nothing written.
# Block images of a restart whose partition the meet changed belong to the OLD partition: blockDiagonalize it again.
function agree!(ps::Vector{HIPPartition{T}}, comm::Union{Nothing,Comm}=nothing;
                valid::Union{Nothing,AbstractVector{Bool}}=nothing) where {T<:LabelT}
    R = length(ps); cx = width!(_ctx(comm), T)
    pP = Ptr{Cvoid}[pointer(p.matrix) for p in ps]
    v = valid === nothing ? C_NULL : Int32[x ? 1 : 0 for x in valid]
    d = Ref{Int64}(0); met = Ref{Int32}(0)
    st = GC.@preserve ps ccall((:sdpsr_agree_partitions, libsdpsr), Cint,
                               (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Int32}, Int64, Ref{Int64}, Ref{Int32}, Cint),
                               cx.handle, _handle(comm), R, pP, v, length(ps[1].matrix), d, met, MEM_HOST)
    check(cx, st)
    if met[] != 0
        for p in ps
            p.nparts = Int(d[])
        end
    end
    return met[] != 0
end

# blockDiagonalize's side (eigen_decomposition.jl:264-270, diagonalize.jl:4-9: "try again" -- the tries ran side by side): the
# lowest rank whose status is 0 wins; returns (winner, its blkSizes), (-1, nothing) when every rank failed.  `capacity`: the same
# on every rank.  The winner's Q_hat travels with broadcast!.
function agree_block_sizes(status::Integer, blk_sizes::AbstractVector{<:Integer}, comm::Union{Nothing,Comm}=nothing; capacity::Integer=65536)
    cx = _ctx(comm); mine = Vector{Int32}(blk_sizes); out = zeros(Int32, capacity)
    w = Ref{Int32}(-1); nb = Ref{Int32}(0)
    check(cx, ccall((:sdpsr_agree_block_diagonalization, libsdpsr), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ref{Int32}, Ref{Int32}, Ptr{Int32}, Int32),
                    cx.handle, _handle(comm), status, length(mine), mine, w, nb, out, capacity))
    return w[] < 0 ? (-1, nothing) : (Int(w[]), Int.(out[1:nb[]]))
end
function broadcast!(buf::Array, comm::Comm; root::Integer=0)
    check(comm.ctx, ccall((:sdpsr_comm_broadcast, libsdpsr), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Cint),
                          comm.ctx.handle, comm.handle, buf, sizeof(buf), root, MEM_HOST))
    return buf
end

end # module
