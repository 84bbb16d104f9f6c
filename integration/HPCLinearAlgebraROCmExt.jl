"""
    HPCLinearAlgebraROCmExt

DeviceROCm extension for HPCLinearAlgebra (sloisel/LinearAlgebraMPI.jl): AMD Instinct MI355X
(gfx950) support through `libhpcla_rocm.so` (C ABI: include/hpcla_rocm.h in this repository).

Install as `ext/HPCLinearAlgebraROCmExt.jl` of the reference package together with the parent
patches listed in INTEGRATION.md (struct DeviceROCm, factory stubs, [weakdeps] AMDGPU).

STATUS: written to the reference's hook contract (the method set of ext/HPCLinearAlgebraCUDAExt.jl:98-187
and ext/HPCLinearAlgebraMetalExt.jl:35-116) but NOT executed -- Julia is not available in the
build environment.  Every `@ccall` below has a tested twin in linearalgebrampi.jl_amd/_capi.py, which
drives the same entry points with the same argument order from Python.

The library path comes from ENV["HPCLA_ROCM_LIB"] (default "libhpcla_rocm").
"""
module HPCLinearAlgebraROCmExt

using HPCLinearAlgebra
using AMDGPU
using MPI
using LinearAlgebra
using SparseArrays

using HPCLinearAlgebra: HPCBackend, DeviceROCm, CommSerial, CommMPI, AbstractComm, SolverMUMPS,
                        VectorRepartitionPlan, AdditionPlan,
                        HPCVector, HPCSparseMatrix, HPCMatrix, VectorPlan,
                        comm_rank, comm_size, indextype_backend, get_vector_plan,
                        compute_partition_hash, assert_backends_compatible

const LIB = get(ENV, "HPCLA_ROCM_LIB", "libhpcla_rocm")
const ROCBackend{T,Ti,C,S} = HPCBackend{T,Ti,DeviceROCm,C,S}

# ---- status convention (cf. ext/HPCLinearAlgebraCUDAExt.jl:248-251) ------------------------------
function _check(status::Cint, what::AbstractString)
    status == 0 || error("$what failed with status $status: " *
                         unsafe_string(@ccall LIB.hpcla_last_error()::Cstring))
    return nothing
end
_stream() = Ptr{Cvoid}(UInt(AMDGPU.stream().stream))          # task-local HIP stream
_ptr(a::ROCArray) = Ptr{Cvoid}(UInt(pointer(a)))
_ptr(::Nothing) = C_NULL
_len(a) = a === nothing ? 0 : length(a)

# partition -> its Blake3 hash (compute_partition_hash, src/HPCLinearAlgebra.jl:255-259), kept by CONTENT: the per-call plan
# lookups of A * B (the key of src/sparse.jl:1992-2001 wants hash(B.row_partition)) and of dense A * x do not hash again
const _partition_hashes = Dict{Vector{Int},Any}()
function _partition_hash(p::Vector{Int})
    h = get(_partition_hashes, p, nothing)
    h === nothing && (h = _partition_hashes[copy(p)] = compute_partition_hash(p))
    return h
end

# ---- backend factories (cf. ext/HPCLinearAlgebraCUDAExt.jl:98-121) ---------------------------------
function HPCLinearAlgebra.backend_rocm_serial(::Type{T}=Float64, ::Type{Ti}=Int) where {T,Ti<:Integer}
    return HPCBackend{T,Ti,DeviceROCm,CommSerial,SolverMUMPS}(DeviceROCm(), CommSerial(), SolverMUMPS())
end
function HPCLinearAlgebra.backend_rocm_mpi(::Type{T}=Float64, ::Type{Ti}=Int;
                                           comm::MPI.Comm=MPI.COMM_WORLD) where {T,Ti<:Integer}
    # one process per GPU: device = rank % ndevices (ext/HPCLinearAlgebraCUDAExt.jl:611-613)
    AMDGPU.device!(AMDGPU.devices()[MPI.Comm_rank(comm) % length(AMDGPU.devices()) + 1])
    return HPCBackend{T,Ti,DeviceROCm,CommMPI,SolverMUMPS}(DeviceROCm(), CommMPI(comm), SolverMUMPS())
end
HPCLinearAlgebra.backend_rocm_mpi(comm::MPI.Comm) = HPCLinearAlgebra.backend_rocm_mpi(Float64, Int; comm=comm)

# ---- array conversion hooks (cf. :129-187) -----------------------------------------------------------
HPCLinearAlgebra._convert_array(v::Vector, ::DeviceROCm) = ROCVector(v)
HPCLinearAlgebra._convert_array(A::Matrix, ::DeviceROCm) = ROCMatrix(A)
HPCLinearAlgebra._convert_array(v::ROCVector, ::DeviceROCm) = v
HPCLinearAlgebra._convert_array(A::ROCMatrix, ::DeviceROCm) = A
HPCLinearAlgebra._zeros_device(::DeviceROCm, ::Type{T}, dims...) where T = AMDGPU.zeros(T, dims...)
HPCLinearAlgebra._index_array_type(::DeviceROCm, ::Type{Ti}) where Ti = ROCVector{Ti}
HPCLinearAlgebra._to_target_device(v::Vector{Ti}, ::DeviceROCm) where Ti = ROCVector(v)
HPCLinearAlgebra._array_to_device(v::Vector{T}, ::DeviceROCm) where T = ROCVector(v)
function HPCLinearAlgebra._convert_vector_to_device(v::HPCVector{T,B}, device::DeviceROCm) where {T,B}
    Ti = indextype_backend(B)
    b = HPCBackend{T,Ti,DeviceROCm,typeof(v.backend.comm),typeof(v.backend.solver)}(
        device, v.backend.comm, v.backend.solver)
    return HPCLinearAlgebra.to_backend(v, b)
end

# ---- RCCL communicator, bootstrapped from MPI (cf. :376-443) -------------------------------------------
# Lives until process exit: no finalizer may issue a collective (:384-386).
const _comms = Dict{Any,Ptr{Cvoid}}()
function _rccl(comm::AbstractComm)
    key = comm isa CommMPI ? comm.comm : :serial
    haskey(_comms, key) && return _comms[key]
    nranks, rank = comm_size(comm), comm_rank(comm)
    id = zeros(UInt8, 128)
    if nranks > 1
        rank == 0 && _check(@ccall(LIB.hpcla_comm_get_unique_id(id::Ptr{UInt8})::Cint), "hpcla_comm_get_unique_id")
        MPI.Bcast!(id, 0, comm.comm)
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    _check(@ccall(LIB.hpcla_comm_init_rank(h::Ptr{Ptr{Cvoid}}, id::Ptr{UInt8}, nranks::Cint, rank::Cint)::Cint),
           "hpcla_comm_init_rank")
    nranks > 1 && _attach_comm_window(h[], comm.comm, nranks)
    return _comms[key] = h[]
end

# ---- peer windows (push transport over xGMI, csrc/window.hip): same bootstrap pattern as the unique id --
# every rank exports a 128-byte descriptor, MPI all-gathers them, every rank attaches; then a connection
# test whose verdict is all-gathered too, so that either every rank uses the windows or none does.
const _windows_ok = Dict{Ptr{Cvoid},Bool}()
function _attach_comm_window(h::Ptr{Cvoid}, mpicomm::MPI.Comm, nranks::Int)
    desc = zeros(UInt8, 128)
    _check(@ccall(LIB.hpcla_comm_window_export(h::Ptr{Cvoid}, desc::Ptr{UInt8})::Cint), "hpcla_comm_window_export")
    descs = MPI.Allgather(desc, mpicomm)
    one_node = all(i -> descs[65 + 128*(i-1) : 72 + 128*(i-1)] == descs[65:72], 1:nranks)   # bytes 64..71: node identity
    ok = Ref{Cint}(0)
    if one_node && (@ccall LIB.hpcla_comm_window_attach(h::Ptr{Cvoid}, descs::Ptr{UInt8})::Cint) == 0
        @ccall LIB.hpcla_comm_window_selftest(h::Ptr{Cvoid}, 10.0::Cdouble, ok::Ptr{Cint})::Cint
    end
    good = minimum(MPI.Allgather(Int32[ok[]], mpicomm)) == 1
    good || _check(@ccall(LIB.hpcla_comm_window_detach(h::Ptr{Cvoid})::Cint), "hpcla_comm_window_detach")
    return _windows_ok[h] = good
end

# plan-time, collective over the communicator (ranks without neighbours pass halo == C_NULL)
# `probe = (n_local_rows, segments)`: segments[i] = 0-based rows of neighbour recv_rank_ids[i] that fill its ghost
# segment, in ghost order -- the plan's connection test (hpcla_halo_plan_probe) checks a sample of them
function _attach_halo_window(h::Ptr{Cvoid}, halo::Ptr{Cvoid}, mpicomm::MPI.Comm, nranks::Int, probe=nothing)
    get(_windows_ok, h, false) || return false
    desc = zeros(UInt8, 128); table = fill(Int64(-1), 4 * nranks)
    halo == C_NULL || _check(@ccall(LIB.hpcla_halo_plan_export(halo::Ptr{Cvoid}, desc::Ptr{UInt8}, table::Ptr{Int64})::Cint),
                             "hpcla_halo_plan_export")
    descs = MPI.Allgather(desc, mpicomm); tables = MPI.Allgather(table, mpicomm)
    mine = halo != C_NULL && any(!=(0x00), desc[81:88])            # bytes 80..87: window size
    ok = !mine || (@ccall LIB.hpcla_halo_plan_attach(halo::Ptr{Cvoid}, descs::Ptr{UInt8}, tables::Ptr{Int64})::Cint) == 0
    attached = minimum(MPI.Allgather(Int32[ok ? 1 : 0], mpicomm)) == 1
    if attached
        # connection test of THIS plan on the real topology: two checked exchanges; verdict all-gathered
        if mine && probe !== nothing
            n_local, segments = probe
            slots = Int64[]; rows = Int64[]; off = 0
            for seg in segments
                cnt = length(seg)
                pick = unique(vcat(1:min(cnt, 2048), max(cnt - 2047, 1):cnt, cnt > 0 ? rand(1:cnt, 8192) : Int[]))
                append!(slots, off .+ pick .- 1); append!(rows, Int64.(seg[pick])); off += cnt
            end
            good = Ref{Cint}(0)
            rc = @ccall LIB.hpcla_halo_plan_probe(halo::Ptr{Cvoid}, Int64(n_local)::Int64, slots::Ptr{Int64}, rows::Ptr{Int64},
                                                  length(slots)::Int64, _stream()::Ptr{Cvoid}, good::Ptr{Cint})::Cint
            ok = rc == 0 && good[] == 1
        end
        attached = minimum(MPI.Allgather(Int32[ok ? 1 : 0], mpicomm)) == 1
    end
    if !attached
        mine && _check(@ccall(LIB.hpcla_halo_plan_detach(halo::Ptr{Cvoid})::Cint), "hpcla_halo_plan_detach")
        return false
    end
    return mine
end

# ---- VectorPlan(A, x) for DeviceROCm: the reference's lists, built without its per-column work ------------------------------
# The parent's constructor (src/sparse.jl:1875-1984) walks A.col_indices once per COLUMN -- one searchsortedlast and one push! of
# a (global, position) tuple each (8.4 M per rank at config 3), then comprehensions over those tuples -- and allocates `gathered`
# (device) plus `gathered_cpu` (host), ncols_compressed values each (64 MiB + 64 MiB per plan at config 3), which the device
# A * x never reads.  col_indices is sorted and owners are contiguous rank ranges, so every owner's columns are ONE contiguous run
# of it: nranks - 1 binary searches find the runs (the twin of sparse.py build_host_vector_plan, whose lists are held equal to the
# oracle's restatement of the parent's constructor at world 2 / 3 / 8).  Same fields, same values, the SAME collectives in the same
# order (Alltoall of the counts, tag-20 index exchange), so ranks may even mix this method with the parent's.  For Float64 -- where
# execute_plan! and mul! are this file's and never touch them -- `gathered` starts empty (execute_plan! below sizes it on first
# use by another caller) and `gathered_cpu` stays empty; other element types keep the parent's buffers (its execute_plan! runs).
function HPCLinearAlgebra.VectorPlan(A::HPCSparseMatrix{T,Ti,B}, x::HPCVector{T,B}) where {T,Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, x.backend)
    comm = A.backend.comm
    rank = comm_rank(comm); nranks = comm_size(comm)
    col_indices = A.col_indices
    n_gathered = length(col_indices)
    my_x_start = x.partition[rank+1]
    # step 1 (:1888-1896): owner(g) = min(searchsortedlast(x.partition, g) - 1, nranks - 1), so owner r holds the columns in
    # [partition[r+1], partition[r+2]) (the last owner: everything from its start on): bounds[r+1]+1 : bounds[r+2] in col_indices
    bounds = Vector{Int}(undef, nranks + 1)
    bounds[1] = 0; bounds[nranks+1] = n_gathered
    for r in 1:(nranks-1); bounds[r+1] = searchsortedfirst(col_indices, x.partition[r+1]) - 1; end
    # step 2 (:1899-1900)
    send_counts = [bounds[r+2] - bounds[r+1] for r in 0:(nranks-1)]
    recv_counts = HPCLinearAlgebra.comm_alltoall(comm, MPI.UBuffer(send_counts, 1))
    # step 3 (:1908-1921): ask every owner for my columns in its slice
    recv_rank_ids = Int[]; recv_perm = Vector{Ti}[]
    struct_send_bufs = Vector{Int}[]; struct_send_reqs = []
    for r in 0:(nranks-1)
        if send_counts[r+1] > 0 && r != rank
            push!(recv_rank_ids, r)
            push!(recv_perm, collect(Ti, (bounds[r+1]+1):bounds[r+2]))               # positions in `gathered`, 1-based
            push!(struct_send_bufs, col_indices[(bounds[r+1]+1):bounds[r+2]])
            push!(struct_send_reqs, HPCLinearAlgebra.comm_isend(comm, struct_send_bufs[end], r, 20))
        end
    end
    # step 4 (:1923-1936)
    send_rank_ids = Int[]; struct_recv_bufs = Vector{Int}[]; struct_recv_reqs = []
    for r in 0:(nranks-1)
        if recv_counts[r+1] > 0 && r != rank
            push!(send_rank_ids, r)
            push!(struct_recv_bufs, Vector{Int}(undef, recv_counts[r+1]))
            push!(struct_recv_reqs, HPCLinearAlgebra.comm_irecv!(comm, struct_recv_bufs[end], r, 20))
        end
    end
    HPCLinearAlgebra.comm_waitall(comm, struct_recv_reqs)
    HPCLinearAlgebra.comm_waitall(comm, struct_send_reqs)
    # step 5 (:1939-1944): global -> local indices of what I send
    send_indices = Vector{Ti}[Ti.(buf .- (my_x_start - 1)) for buf in struct_recv_bufs]
    # step 6 (:1947-1953): the columns I own myself
    lo, hi = bounds[rank+1] + 1, bounds[rank+2]
    local_src_indices = Ti.(col_indices[lo:hi] .- (my_x_start - 1))
    local_dst_indices = collect(Ti, lo:hi)
    # step 7 (:1956-1984; both rank lists are ascending by construction)
    send_bufs = [Vector{T}(undef, length(inds)) for inds in send_indices]
    recv_bufs = [Vector{T}(undef, send_counts[r+1]) for r in recv_rank_ids]
    send_reqs = Vector{Any}(undef, length(send_rank_ids))
    recv_reqs = Vector{Any}(undef, length(recv_rank_ids))
    lazy = T === Float64
    gathered_cpu = Vector{T}(undef, lazy ? 0 : n_gathered)
    gathered = similar(x.v, lazy ? 0 : n_gathered)
    AV = typeof(x.v)
    return VectorPlan{T,Ti,AV}(
        send_rank_ids, send_indices, send_bufs, send_reqs,
        recv_rank_ids, recv_bufs, recv_reqs, recv_perm,
        local_src_indices, local_dst_indices, gathered, gathered_cpu,
        nothing, nothing,
        nothing, nothing,
        nothing, nothing)
end

# ---- device half of the VectorPlan, cached next to the reference plan -----------------------------------
# Tk = index type of the KERNEL arrays of the plan.  The parent's default is Ti = Int (src/backends.jl:348,369), so a
# caller who follows the defaults hands over Int64 structure arrays although every realistic per-GPU share fits Int32.
# Indices are never results: when nnz and the split column space (own offsets, then positions in the ghost segment)
# fit, the plan keeps Int32 copies (hpcla_remap_i64_to_i32, hpcla_narrow_i64_to_i32) and every launch over it takes
# the _i32 kernels -- 12 instead of 16 bytes per stored entry, the same bits of y.  A and its arrays keep their type.
# HPCLA_NARROW_INDICES=0 keeps Int64 structures on the Int64 kernels.
mutable struct ROCVectorPlan{Tk}
    halo::Ptr{Cvoid}                 # hpcla_halo_plan_t* (C_NULL when there are no neighbours)
    colval_split::ROCVector{Tk}      # 0-based split columns: < n_own -> x.v, >= n_own -> ghost segment
    rowptr0::ROCVector{Tk}           # 0-based rowptr of the kernels (equal for every matrix that shares the plan: the
                                     # structural hash covers rowptr); carries the block-order hint
    interior::ROCVector{Int32}
    boundary::ROCVector{Int32}
    n_own::Int
    segments::Vector{Vector{Int}}    # per recv neighbour: 0-based rows (in their owner) that fill its ghost segment
end
const _rocm_plans = IdDict{Any,Any}()    # reference plan object -> ROCVectorPlan (freed by clear_rocm_plan_cache!)

# everything an index array of the plan can hold must fit Int32 (0-based arrays: rowptr reaches nnz, split columns
# n_own + n_ghost - 1, send indices n_own - 1)
_can_narrow(nnz, nrows, n_own, n_ghost) =
    get(ENV, "HPCLA_NARROW_INDICES", "1") != "0" && nnz <= typemax(Int32) && nrows <= typemax(Int32) &&
    n_own + n_ghost <= typemax(Int32)
_kernel_index_type(::Type{Int32}, nnz, nrows, n_own, n_ghost) = Int32
_kernel_index_type(::Type{Int64}, nnz, nrows, n_own, n_ghost) = _can_narrow(nnz, nrows, n_own, n_ghost) ? Int32 : Int64

_device_plan(A::HPCSparseMatrix{T,Ti,B}, x::HPCVector{T,B}, plan) where {T,Ti,B<:ROCBackend} =
    _device_plan(A, x.partition, length(x.v), _ptr(x.v), plan)
# `xpart`, `n_own`: the partition of the operand and this rank's share of it; `xptr`: n_own readable values of the operand's
# type on the device (the block-order measurement multiplies by them and discards the products) or C_NULL -- A * B hands
# over B's row partition and its first column, so no vector is allocated to describe an operand (round 6)
function _device_plan(A::HPCSparseMatrix{T,Ti,B}, xpart::Vector{Int}, n_own::Int, xptr::Ptr{Cvoid}, plan) where {T,Ti,B<:ROCBackend}
    get!(_rocm_plans, plan) do
        nnz = length(A.nzval)
        n_ghost = sum(length, plan.recv_perm; init=0)
        Tk = _kernel_index_type(Ti, nnz, A.nrows_local, n_own, n_ghost)
        # compressed column -> split column (0-based): own columns map to their offset in x.v,
        # ghosts to n_own + position in the ghost segment (recv_perm order == ascending global column)
        cmap = Vector{Tk}(undef, length(A.col_indices))
        cmap[plan.local_dst_indices] .= Tk.(plan.local_src_indices .- one(Ti))
        off = n_own
        for perm in plan.recv_perm
            cmap[perm] .= Tk.(off .+ (0:length(perm)-1)); off += length(perm)
        end
        split = _split_colval(A, cmap)
        # The split-column copy is 0-based while A.rowptr_target keeps the reference's 1-based values; the SpMV entry
        # points apply ONE index_base to rowptr and colval alike, so the plan keeps a 0-based rowptr copy (in Tk) and
        # every kernel over the plan is called with index_base = 0.
        rp0_wide = A.rowptr_target .- one(Ti)
        rp0 = if Tk === Ti
            rp0_wide
        else
            narrow = ROCVector{Int32}(undef, length(rp0_wide)); ovf = AMDGPU.zeros(UInt32, 1)
            _check(@ccall(LIB.hpcla_narrow_i64_to_i32(_ptr(rp0_wide)::Ptr{Cvoid}, _ptr(narrow)::Ptr{Cvoid},
                   length(rp0_wide)::Int64, _ptr(ovf)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_narrow_i64_to_i32")
            Array(ovf)[1] == 0 || error("HPCLinearAlgebraROCmExt: rowptr does not fit Int32")
            narrow
        end
        halo = Ref{Ptr{Cvoid}}(C_NULL)
        segments = [Int.(A.col_indices[perm] .- xpart[r + 1])             # 0-based row in its owner (rank r, 0-based)
                    for (r, perm) in zip(plan.recv_rank_ids, plan.recv_perm)]
        interior = ROCVector{Int32}(undef, 0); boundary = ROCVector{Int32}(undef, 0)
        if !isempty(plan.send_rank_ids) || !isempty(plan.recv_rank_ids)
            send_idx = ROCVector(Tk.(reduce(vcat, plan.send_indices; init=Ti[]) .- one(Ti)))   # 0-based, the kernels' type
            AMDGPU.synchronize()
            # Float32 plans (csrc/f32.hip) are driven through hpcla_halo_begin_f32 / hpcla_halo_end with the ghost pointer
            # taken from the host in between: one ghost buffer (flags = HPCLA_HALO_SINGLE_BUFFER), a constant of the plan
            _check(@ccall(LIB.hpcla_halo_plan_create_ex(halo::Ptr{Ptr{Cvoid}}, _rccl(A.backend.comm)::Ptr{Cvoid},
                   length(plan.send_rank_ids)::Cint, Int32.(plan.send_rank_ids)::Ptr{Int32},
                   Int64.(length.(plan.send_indices))::Ptr{Int64}, _ptr(send_idx)::Ptr{Cvoid},
                   (Tk === Int64 ? 1 : 0)::Cint, length(plan.recv_rank_ids)::Cint,
                   Int32.(plan.recv_rank_ids)::Ptr{Int32}, Int64.(length.(plan.recv_perm))::Ptr{Int64},
                   1::Cint, (T === Float32 ? 1 : 0)::Cint)::Cint), "hpcla_halo_plan_create_ex")
            # `split` is 0-based (hpcla_remap output) while A.rowptr_target is 1-based: the classifier applies
            # ONE index_base to both arrays, so it gets the 0-based rowptr copy and index_base = 0 -- with
            # base 1 the first ghost column (== n_own) would count as owned and its row block as interior
            interior, boundary = _classify_blocks(A, rp0, split, n_own, (@ccall LIB.hpcla_spmv_rows_per_block()::Cint))
        end
        # collective: map the neighbours' ghost windows (push transport); a no-op without attached windows
        A.backend.comm isa CommMPI &&
            _attach_halo_window(_rccl(A.backend.comm), halo[], A.backend.comm.comm, comm_size(A.backend.comm),
                                (n_own, segments))
        # Block order of this matrix's SpMV launches, MEASURED once here (hpcla_spmv_tune_block_order_*: 64 launches of
        # the split-column SpMV into a scratch vector; the library keeps the fastest order registered for the rowptr
        # array the launches use -- the plan's 0-based copy).  No reference counterpart: a performance setting only,
        # every order gives the same bits.
        if T === Float64 && A.nrows_local > 0 && nnz > 0 && xptr != C_NULL
            scratch = similar(A.nzval, A.nrows_local)
            gh = Ref{Ptr{Cvoid}}(C_NULL); ngh = Ref{Int64}(0)
            halo[] != C_NULL &&
                _check(@ccall(LIB.hpcla_halo_ghost_ptr(halo[]::Ptr{Cvoid}, gh::Ptr{Ptr{Cvoid}}, ngh::Ptr{Int64})::Cint), "hpcla_halo_ghost_ptr")
            chosen = Ref{Cint}(1)
            if Tk === Int32
                _check(@ccall(LIB.hpcla_spmv_tune_block_order_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(split)::Ptr{Cvoid},
                       _ptr(A.nzval)::Ptr{Cvoid}, xptr::Ptr{Cvoid}, gh[]::Ptr{Cvoid}, n_own::Int64, _ptr(scratch)::Ptr{Cvoid},
                       A.nrows_local::Int64, nnz::Int64, 0::Cint, _stream()::Ptr{Cvoid}, chosen::Ptr{Cint})::Cint),
                       "hpcla_spmv_tune_block_order_f64_i32")
            else
                _check(@ccall(LIB.hpcla_spmv_tune_block_order_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(split)::Ptr{Cvoid},
                       _ptr(A.nzval)::Ptr{Cvoid}, xptr::Ptr{Cvoid}, gh[]::Ptr{Cvoid}, n_own::Int64, _ptr(scratch)::Ptr{Cvoid},
                       A.nrows_local::Int64, nnz::Int64, 0::Cint, _stream()::Ptr{Cvoid}, chosen::Ptr{Cint})::Cint),
                       "hpcla_spmv_tune_block_order_f64_i64")
            end
        end
        ROCVectorPlan{Tk}(halo[], split, rp0, interior, boundary, n_own, segments)
    end
end

function _spmv_dist!(y::ROCVector{T}, A::HPCSparseMatrix{T,Ti,B}, x::HPCVector{T,B}) where {T<:Float64,Ti,B<:ROCBackend}
    plan = get_vector_plan(A, x)                   # reference host plan, memoized (src/sparse.jl:1992-2001)
    d = _device_plan(A, x, plan)
    rp0 = d.rowptr0
    nnz = length(A.nzval)
    if eltype(rp0) === Int32                       # the PLAN's index type: Int32 also for a narrowed Int64 matrix
        _check(@ccall(LIB.hpcla_spmv_dist_f64_i32(d.halo::Ptr{Cvoid}, _ptr(rp0)::Ptr{Cvoid},
               _ptr(d.colval_split)::Ptr{Cvoid}, _ptr(A.nzval)::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, d.n_own::Int64,
               _ptr(y)::Ptr{Cvoid}, A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(d.interior)::Ptr{Cvoid},
               length(d.interior)::Int64, _ptr(d.boundary)::Ptr{Cvoid}, length(d.boundary)::Int64,
               _stream()::Ptr{Cvoid})::Cint), "hpcla_spmv_dist_f64_i32")
    else
        _check(@ccall(LIB.hpcla_spmv_dist_f64_i64(d.halo::Ptr{Cvoid}, _ptr(rp0)::Ptr{Cvoid},
               _ptr(d.colval_split)::Ptr{Cvoid}, _ptr(A.nzval)::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, d.n_own::Int64,
               _ptr(y)::Ptr{Cvoid}, A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(d.interior)::Ptr{Cvoid},
               length(d.interior)::Int64, _ptr(d.boundary)::Ptr{Cvoid}, length(d.boundary)::Int64,
               _stream()::Ptr{Cvoid})::Cint), "hpcla_spmv_dist_f64_i64")
    end
    return plan
end

# ---- A * x  (replaces src/sparse.jl:2096-2128 for DeviceROCm) ---------------------------------------------
function Base.:*(A::HPCSparseMatrix{T,Ti,B}, x::HPCVector{T,B}) where {T<:Float64,Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, x.backend)
    y_local = similar(A.nzval, A.nrows_local)
    plan = _spmv_dist!(y_local, A, x)
    if plan.result_partition_hash === nothing
        plan.result_partition_hash = compute_partition_hash(A.row_partition)
        plan.result_partition = copy(A.row_partition)
    end
    return HPCVector{T,B}(plan.result_partition_hash, plan.result_partition, y_local, A.backend)
end

# ---- mul!(y, A, x)  (replaces the CPU multiply of src/sparse.jl:2019-2037) --------------------------------
function LinearAlgebra.mul!(y::HPCVector{T,B}, A::HPCSparseMatrix{T,Ti,B}, x::HPCVector{T,B}) where {T<:Float64,Ti,B<:ROCBackend}
    _spmv_dist!(y.v, A, x)
    return y
end

# ---- dot / norm  (replace src/vectors.jl:798-812, 758-780) ------------------------------------------------
const _work = Ref{Any}(nothing)
function _scratch()
    _work[] === nothing && (_work[] = (AMDGPU.zeros(UInt8, @ccall LIB.hpcla_reduce_work_bytes()::Int64), AMDGPU.zeros(Float64, 1)))
    return _work[]
end
function LinearAlgebra.dot(x::HPCVector{T,B}, y::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend}
    assert_backends_compatible(x.backend, y.backend)
    x.structural_hash == y.structural_hash || (y = HPCLinearAlgebra.repartition(y, x.partition))   # PCIe: none -- lands in this file's execute_plan!(::VectorRepartitionPlan): GPU to GPU
    work, out = _scratch()
    _check(@ccall(LIB.hpcla_dot_f64(_rccl(x.backend.comm)::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, _ptr(y.v)::Ptr{Cvoid},
           length(x.v)::Int64, _ptr(out)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_dot_f64")
    return _host_scalar(out, x.backend)
end
function LinearAlgebra.norm(v::HPCVector{T,B}, p::Real=2) where {T<:Float64,B<:ROCBackend}
    work, out = _scratch(); c = _rccl(v.backend.comm); n = length(v.v)
    if p == 2
        _check(@ccall(LIB.hpcla_nrm2sq_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_nrm2sq_f64")
        return sqrt(_host_scalar(out, v.backend))
    elseif p == 1
        _check(@ccall(LIB.hpcla_asum_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_asum_f64")
        return _host_scalar(out, v.backend)
    elseif p == Inf
        _check(@ccall(LIB.hpcla_amax_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_amax_f64")
        return _host_scalar(out, v.backend)
    else
        p > 0 || return invoke(LinearAlgebra.norm, Tuple{HPCVector,Real}, v, p)     # PCIe: parent's generic method (p <= 0 only) -- whatever the array package's norm moves
        _check(@ccall(LIB.hpcla_powsum_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, Float64(p)::Cdouble,
               _ptr(out)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_powsum_f64")
        return _host_scalar(out, v.backend)^(1 / p)
    end
end

# ---- u + v, u - v, -v, a * v, v * a, v / a  (replace src/vectors.jl:868-903, 944-964 for Float64 vectors on DeviceROCm) -------
# The parent's methods broadcast over `.v` (AMDGPU.jl's generic broadcast kernel); these bind the row's own kernels (csrc/vecops.hip:
# 16-byte loads, grid sized for the chip) with the parent's semantics -- the result has u's partition and hash, a vector on another
# partition is repartitioned first (the device exchange of execute_plan!(::VectorRepartitionPlan) below).  Same bits: 1 * u[i] and
# -1 * v[i] are exact, so axpby(1, u, +-1, v) rounds once, like u[i] +- v[i].  General broadcast (`u .+ a .* v`) stays AMDGPU.jl's.
# (Bool stays with the parent's broadcast: `false * x` is a STRONG zero in Julia -- false * NaN == 0.0 -- which 0.0 * x is not)
const _HostReal = Union{Float64,Float32,Float16,Int8,Int16,Int32,Int64,UInt8,UInt16,UInt32,UInt64}    # promote_type(., Float64) == Float64
function _axpby(a::Float64, u::HPCVector{T,B}, b::Float64, v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend}
    assert_backends_compatible(u.backend, v.backend)
    u.structural_hash == v.structural_hash || (v = HPCLinearAlgebra.repartition(v, u.partition))   # PCIe: none -- lands in this file's execute_plan!(::VectorRepartitionPlan): GPU to GPU
    out = similar(u.v)
    _check(@ccall(LIB.hpcla_axpby_f64(a::Cdouble, _ptr(u.v)::Ptr{Cvoid}, b::Cdouble, _ptr(v.v)::Ptr{Cvoid}, _ptr(out)::Ptr{Cvoid},
           length(out)::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_axpby_f64")
    return HPCVector{T,B}(u.structural_hash, u.partition, out, u.backend)
end
Base.:+(u::HPCVector{T,B}, v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _axpby(1.0, u, 1.0, v)
Base.:-(u::HPCVector{T,B}, v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _axpby(1.0, u, -1.0, v)
function _scaled(a::Float64, v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend}
    out = similar(v.v)
    _check(@ccall(LIB.hpcla_scale_f64(a::Cdouble, _ptr(v.v)::Ptr{Cvoid}, _ptr(out)::Ptr{Cvoid}, length(out)::Int64,
           _stream()::Ptr{Cvoid})::Cint), "hpcla_scale_f64")
    return HPCVector{T,B}(v.structural_hash, v.partition, out, v.backend)
end
Base.:-(v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _scaled(-1.0, v)
Base.:*(a::_HostReal, v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _scaled(Float64(a), v)
Base.:*(v::HPCVector{T,B}, a::_HostReal) where {T<:Float64,B<:ROCBackend} = _scaled(Float64(a), v)
function Base.:/(v::HPCVector{T,B}, a::_HostReal) where {T<:Float64,B<:ROCBackend}
    out = similar(v.v)                                   # a true division per element, like `v.v ./ a` (not a reciprocal multiply)
    _check(@ccall(LIB.hpcla_divide_f64(_ptr(v.v)::Ptr{Cvoid}, Float64(a)::Cdouble, _ptr(out)::Ptr{Cvoid}, length(out)::Int64,
           _stream()::Ptr{Cvoid})::Cint), "hpcla_divide_f64")
    return HPCVector{T,B}(v.structural_hash, v.partition, out, v.backend)
end

# A NaN that reaches the host may be the POISON of an expired exchange wait (the kernels never compute from stale
# ghosts: rows / partials / all-reduce results that depended on a neighbour that did not show up within
# HPCLA_PUSH_TIMEOUT_S become NaN, and the plan's sticky status word is set).  The reference's MPI exchange would
# block instead (src/vectors.jl:446); here the failure is turned into an error wherever a scalar is read back.
function _check_exchange_health(backend)
    flag = Ref{Cint}(0)
    c = _rccl(backend.comm)
    if c != C_NULL
        _check(@ccall(LIB.hpcla_comm_status(c::Ptr{Cvoid}, flag::Ptr{Cint})::Cint), "hpcla_comm_status")
        flag[] == 0 || error("HPCLinearAlgebraROCmExt: a window all-reduce timed out (a rank did not arrive within HPCLA_PUSH_TIMEOUT_S)")
    end
    for d in values(_rocm_plans)
        d isa ROCVectorPlan && d.halo != C_NULL || continue
        _check(@ccall(LIB.hpcla_halo_status(d.halo::Ptr{Cvoid}, flag::Ptr{Cint})::Cint), "hpcla_halo_status")
        flag[] == 0 || error("HPCLinearAlgebraROCmExt: a halo exchange timed out; the affected results are NaN")
    end
    # the width-k plans of A * B and the device exchanges of execute_plan! poison their ghost buffers the same way
    for (what, cache) in (("an SpMM ghost-row exchange", _spmm_plans), ("an execute_plan! exchange", _rocm_exec),
                          ("the value exchange of a sparse A * B", _rocm_matexec))
        for st in values(cache)
            st[1] == C_NULL && continue
            _check(@ccall(LIB.hpcla_halo_status(st[1]::Ptr{Cvoid}, flag::Ptr{Cint})::Cint), "hpcla_halo_status")
            flag[] == 0 || error("HPCLinearAlgebraROCmExt: $what timed out; the affected results are NaN")
        end
    end
    return nothing
end
function _host_scalar(out, backend)
    v = Array(out)[1]                           # PCIe: 8 B -- the scalar result itself (the reference returns a host number)
    isnan(v) && _check_exchange_health(backend)
    return v
end

# ---- k fused CG iterations in ONE library call (the reference has no Krylov solver, SURVEY 3.4: a caller composes
# the iteration from A*p src/sparse.jl:2096-2128, dot src/vectors.jl:798-812, the broadcasts :1203-1226 and norm
# :758-765; this is that composition with neither Julia nor Python inside the loop).  x0 = 0, r0 = p0 = b;
# returns (x, [norm(r_0), ..., norm(r_iters)]).
function rocm_cg_iterations(A::HPCSparseMatrix{T,Ti,B}, b::HPCVector{T,B}, iters::Integer) where {T<:Float64,Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, b.backend)
    plan = get_vector_plan(A, b)
    d = _device_plan(A, b, plan)
    d.n_own == A.nrows_local || error("rocm_cg_iterations: b must be partitioned like the rows of A")
    n = A.nrows_local
    x = AMDGPU.zeros(T, n); r = copy(b.v); p = copy(b.v); Ap = similar(b.v)
    hist = AMDGPU.zeros(T, iters + 1); pAp = AMDGPU.zeros(T, 1)
    work, _ = _scratch()
    dot_work = AMDGPU.zeros(UInt8, @ccall LIB.hpcla_spmv_dot_work_bytes(n::Int64)::Int64)
    c = _rccl(A.backend.comm)
    _check(@ccall(LIB.hpcla_nrm2sq_f64(c::Ptr{Cvoid}, _ptr(r)::Ptr{Cvoid}, n::Int64, _ptr(hist)::Ptr{Cvoid},
           _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_nrm2sq_f64")          # hist[1] = sum r0^2
    rp0 = d.rowptr0; nnz = length(A.nzval)
    if eltype(rp0) === Int32
        _check(@ccall(LIB.hpcla_cg_iterations_f64_i32(d.halo::Ptr{Cvoid}, c::Ptr{Cvoid}, _ptr(rp0)::Ptr{Cvoid},
               _ptr(d.colval_split)::Ptr{Cvoid}, _ptr(A.nzval)::Ptr{Cvoid}, n::Int64, nnz::Int64, 0::Cint,
               _ptr(d.interior)::Ptr{Cvoid}, length(d.interior)::Int64, _ptr(d.boundary)::Ptr{Cvoid},
               length(d.boundary)::Int64, _ptr(x)::Ptr{Cvoid}, _ptr(r)::Ptr{Cvoid}, _ptr(p)::Ptr{Cvoid}, _ptr(Ap)::Ptr{Cvoid},
               _ptr(hist)::Ptr{Cvoid}, _ptr(pAp)::Ptr{Cvoid}, _ptr(dot_work)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid},
               Cint(iters)::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_cg_iterations_f64_i32")
    else
        _check(@ccall(LIB.hpcla_cg_iterations_f64_i64(d.halo::Ptr{Cvoid}, c::Ptr{Cvoid}, _ptr(rp0)::Ptr{Cvoid},
               _ptr(d.colval_split)::Ptr{Cvoid}, _ptr(A.nzval)::Ptr{Cvoid}, n::Int64, nnz::Int64, 0::Cint,
               _ptr(d.interior)::Ptr{Cvoid}, length(d.interior)::Int64, _ptr(d.boundary)::Ptr{Cvoid},
               length(d.boundary)::Int64, _ptr(x)::Ptr{Cvoid}, _ptr(r)::Ptr{Cvoid}, _ptr(p)::Ptr{Cvoid}, _ptr(Ap)::Ptr{Cvoid},
               _ptr(hist)::Ptr{Cvoid}, _ptr(pAp)::Ptr{Cvoid}, _ptr(dot_work)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid},
               Cint(iters)::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_cg_iterations_f64_i64")
    end
    h = sqrt.(Array(hist))                      # PCIe: 8 (iters + 1) B -- the residual history this function returns
    any(isnan, h) && _check_exchange_health(A.backend)
    return HPCVector{T,B}(b.structural_hash, b.partition, x, A.backend), h
end

# sum / prod / maximum / minimum (src/vectors.jl:815-858): same two-stage device reduction + scalar all-reduce
function _reduce_scalar(sym::Symbol, v::HPCVector, negate::Int=0)
    work, out = _scratch(); c = _rccl(v.backend.comm); n = length(v.v)
    if sym === :sum
        _check(@ccall(LIB.hpcla_sum_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_sum_f64")
    elseif sym === :prod
        _check(@ccall(LIB.hpcla_prod_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_prod_f64")
    else
        _check(@ccall(LIB.hpcla_maxval_f64(c::Ptr{Cvoid}, _ptr(v.v)::Ptr{Cvoid}, n::Int64, negate::Cint, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_maxval_f64")
    end
    return _host_scalar(out, v.backend)
end
Base.sum(v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _reduce_scalar(:sum, v)
Base.prod(v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _reduce_scalar(:prod, v)
Base.maximum(v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = _reduce_scalar(:max, v, 0)
Base.minimum(v::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend} = -_reduce_scalar(:max, v, 1)      # min x = -max(-x)

# ---- A * B, B::HPCMatrix  (replaces the column loop of src/sparse.jl:2391-2413) ---------------------------
# Julia's Matrix is column-major.  BANDED structures (every stencil) are multiplied on the column-major blocks as they are
# (_spmm_colmajor below: lanes = rows, a wave reads one contiguous run of a column per gather instruction).  Unstructured
# matrices would touch a line per (entry, column) pair in that layout; for them the fast layout is row-major (one 128-byte
# line per B row at k = 16), so B is converted once with hpcla_transpose_f64; C leaves the product column-major.
const _spmm_plans = IdDict{Any,Any}()     # (reference plan, width, rows per block) -> (halo handle, interior, boundary, send_idx, ghost pointer, colval_split, rowptr0); freed by clear_rocm_plan_cache!

# The result of A * B as the parent's HPCMatrix_local would describe it (src/dense.jl:125-156): A's row partition (its Allgather of
# the local row counts returns exactly diff(A.row_partition)), the default column partition, lazy hash -- WITHOUT its
# `Matrix(A_local)` (src/dense.jl:153): for a ROCMatrix that is a device -> host copy of the whole product, followed by the
# host -> device copy of _convert_array, around a product that never left the device (268 MB each way at config 5's share).
# A * x returns through the inner constructor for the same reason (src/sparse.jl:2122-2127).
_spmm_result(A::HPCSparseMatrix{T,Ti,B}, C::ROCMatrix{T}, k::Int) where {T,Ti,B} =
    HPCMatrix{T,B}(nothing, copy(A.row_partition), HPCLinearAlgebra.uniform_partition(k, comm_size(A.backend.comm)), C, A.backend)

# The vector plan for (A, B's row partition) provides the neighbour lists and the split column space.  Its lookup key
# (src/sparse.jl:1992-2001) reads the partition hash and typeof(x.v) only: the probe carries a ZERO-length vector, the device
# half takes its sizes from B itself (round 6: was a full-length device allocation per product, only to key the lookup).
function _spmm_vector_plan(A::HPCSparseMatrix{T,Ti,B}, M::HPCMatrix{T,B}) where {T,Ti,B<:ROCBackend}
    nloc, k = size(M.A)
    probe = HPCVector{T,B}(_partition_hash(M.row_partition), M.row_partition, similar(A.nzval, 0), A.backend)   # plan key only
    plan = get_vector_plan(A, probe)
    # (B's first column is nloc contiguous values: what the plan's block-order measurement reads)
    d = _device_plan(A, M.row_partition, nloc, (k > 0 && nloc > 0) ? _ptr(M.A) : C_NULL, plan)
    d.n_own == nloc || error("A * B: B's local rows do not match its row partition")
    return plan, d
end

# split-column copy of A's colval through the compressed-column map `cmap` (0-based values in the kernels' index type Tk):
# hpcla_remap_* in A's index type, or narrowing on the fly
function _split_colval(A::HPCSparseMatrix{T,Ti,B}, cmap::Vector{Tk}) where {T,Ti,Tk,B}
    nnz = length(A.nzval)
    cmap_d = ROCVector(cmap)
    split = ROCVector{Tk}(undef, nnz)
    if Ti === Int32
        _check(@ccall(LIB.hpcla_remap_i32(_ptr(A.colval_target)::Ptr{Cvoid}, _ptr(cmap_d)::Ptr{Cvoid},
               _ptr(split)::Ptr{Cvoid}, nnz::Int64, 1::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_remap_i32")
    elseif Tk === Int64
        _check(@ccall(LIB.hpcla_remap_i64(_ptr(A.colval_target)::Ptr{Cvoid}, _ptr(cmap_d)::Ptr{Cvoid},
               _ptr(split)::Ptr{Cvoid}, nnz::Int64, 1::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_remap_i64")
    else        # Int64 matrix, narrowed arrays: Int64 compressed columns in, Int32 split columns out
        _check(@ccall(LIB.hpcla_remap_i64_to_i32(_ptr(A.colval_target)::Ptr{Cvoid}, _ptr(cmap_d)::Ptr{Cvoid},
               _ptr(split)::Ptr{Cvoid}, nnz::Int64, 1::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_remap_i64_to_i32")
    end
    AMDGPU.synchronize()                                    # cmap_d is read by the kernel above
    return split
end

# interior / boundary lists of the `rpb`-row blocks (hpcla_classify_blocks_*: 0-based arrays, index_base = 0)
function _classify_blocks(A, rp0::ROCVector{Tk}, colval_split::ROCVector{Tk}, n_own::Int, rpb::Cint) where {Tk}
    flags = AMDGPU.zeros(Int32, cld(A.nrows_local, rpb))
    if Tk === Int32
        _check(@ccall(LIB.hpcla_classify_blocks_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               A.nrows_local::Int64, 0::Cint, n_own::Int64, rpb::Cint, _ptr(flags)::Ptr{Cvoid},
               _stream()::Ptr{Cvoid})::Cint), "hpcla_classify_blocks_i32")
    else
        _check(@ccall(LIB.hpcla_classify_blocks_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               A.nrows_local::Int64, 0::Cint, n_own::Int64, rpb::Cint, _ptr(flags)::Ptr{Cvoid},
               _stream()::Ptr{Cvoid})::Cint), "hpcla_classify_blocks_i64")
    end
    f = Array(flags)
    return ROCVector(Int32.(findall(==(0), f) .- 1)), ROCVector(Int32.(findall(!=(0), f) .- 1))
end

# WHOLE SLICES (SURVEY 8e(3); the twin of linearalgebrampi.jl_amd/sparse.py whole_slice_wishes / whole_slice_lists, executed
# there at world 2 / 3 / 8).  An unstructured A (config 5) touches ~98 % of every other rank's rows of B: gathering and packing
# the requested rows costs the owner a full extra pass over them, an index list as long as its slice (7 x 2.05 M indices per
# product at 8 GPUs) and a send buffer as large as the slice.  A rank that needs more than half of a neighbour's slice asks
# for ALL of it: the owner sends its rows in place order (index list 0:n_own-1), the ghost segment of that neighbour then
# holds its whole slice and column g sits at g - partition[owner] in it.  wish[r + 1] == 1: this rank wants rank r's whole slice.
const _WHOLE_SLICE_FRACTION = 0.5
function _whole_slice_wishes(plan, xpart::Vector{Int}, nranks::Int)
    wish = zeros(Int, nranks)
    for (r, perm) in zip(plan.recv_rank_ids, plan.recv_perm)
        length(perm) > _WHOLE_SLICE_FRACTION * (xpart[r + 2] - xpart[r + 1]) && (wish[r + 1] = 1)
    end
    return wish
end

# width-`width` halo plan for the ghost ROWS of B: the reference VectorPlan's own lists (or whole slices, above), `width`
# values per index (row-major rows travel as contiguous runs of `width` doubles: k, or the padded pitch k + 1 of an odd k).
# COLLECTIVE on first use (an Alltoall of the wishes and the window attach): every rank of the communicator calls it, with or
# without neighbours -- a rank without neighbours gets an entry whose halo handle is C_NULL.
# `rpb`: rows per block of the kernels that will take the interior / boundary lists (the row-major Float64 kernels of
# spmm.hip: hpcla_spmm_rows_per_block(); the lanes = rows kernels -- column-major blocks, Float32 --: the SpMV's 256).
# The entry carries the colval / rowptr arrays ITS kernels read: the vector plan's, unless whole slices moved the ghost positions.
function _spmm_halo(A::HPCSparseMatrix{T,Ti,B}, plan, d::ROCVectorPlan{Tk}, xpart::Vector{Int}, width::Int, rpb::Cint) where {T,Ti,Tk,B<:ROCBackend}
    get!(_spmm_plans, (plan, width, rpb)) do
        comm = A.backend.comm; nranks = comm_size(comm)
        n_own = d.n_own; nnz = length(A.nzval)
        wish = _whole_slice_wishes(plan, xpart, nranks)
        granted = HPCLinearAlgebra.comm_alltoall(comm, MPI.UBuffer(wish, 1))       # granted[q + 1] == 1: rank q gets my whole slice
        if isempty(plan.send_rank_ids) && isempty(plan.recv_rank_ids)
            comm isa CommMPI && _attach_halo_window(_rccl(comm), C_NULL, comm.comm, nranks)   # collective: the other ranks' plans attach
            return (C_NULL, ROCVector{Int32}(undef, 0), ROCVector{Int32}(undef, 0), nothing, C_NULL, d.colval_split, d.rowptr0)
        end
        send_lists = Vector{Ti}[granted[q + 1] == 1 ? collect(Ti, 0:n_own-1) : idx .- one(Ti)
                                for (q, idx) in zip(plan.send_rank_ids, plan.send_indices)]               # 0-based
        recv_counts = Int64[wish[r + 1] == 1 ? xpart[r + 2] - xpart[r + 1] : length(perm)
                            for (r, perm) in zip(plan.recv_rank_ids, plan.recv_perm)]
        n_ghost = sum(recv_counts; init=Int64(0))
        colval_split = d.colval_split; rp0 = d.rowptr0; Tke = Tk
        segments = d.segments
        if any(==(1), wish)
            # ghost positions differ from the vector plan's: a split-column copy of this entry's own -- in the plan's index type,
            # or, when whole slices outgrow a narrowed plan's Int32, in the matrix's
            Tke = _kernel_index_type(Ti, nnz, A.nrows_local, n_own, n_ghost)
            n_own + n_ghost <= typemax(Tke) || error("A * B: the split column space does not fit the index type")
            cmap = Vector{Tke}(undef, length(A.col_indices))
            cmap[plan.local_dst_indices] .= Tke.(plan.local_src_indices .- one(Ti))
            off = n_own
            for (r, perm, cnt) in zip(plan.recv_rank_ids, plan.recv_perm, recv_counts)
                if wish[r + 1] == 1
                    cmap[perm] .= Tke.(off .+ (A.col_indices[perm] .- xpart[r + 1]))      # its row in the owner's slice
                else
                    cmap[perm] .= Tke.(off .+ (0:length(perm)-1))
                end
                off += cnt
            end
            colval_split = _split_colval(A, cmap)
            rp0 = Tke === Tk ? d.rowptr0 : A.rowptr_target .- one(Ti)
            segments = [wish[r + 1] == 1 ? collect(0:(xpart[r + 2] - xpart[r + 1] - 1)) : seg
                        for (r, seg) in zip(plan.recv_rank_ids, d.segments)]
        end
        halo = Ref{Ptr{Cvoid}}(C_NULL)
        send_idx = ROCVector(Tke.(reduce(vcat, send_lists; init=Ti[])))
        AMDGPU.synchronize()
        # flags = 1 (HPCLA_HALO_SINGLE_BUFFER): this plan is driven through halo_begin / halo_end and its consumers
        # take the ghost pointer from the host while the exchange is in flight, so a one-column B (width 1) must
        # not be double-buffered like the fused SpMV's vector plans
        _check(@ccall(LIB.hpcla_halo_plan_create_ex(halo::Ptr{Ptr{Cvoid}}, _rccl(comm)::Ptr{Cvoid},
               length(plan.send_rank_ids)::Cint, Int32.(plan.send_rank_ids)::Ptr{Int32},
               Int64.(length.(send_lists))::Ptr{Int64}, _ptr(send_idx)::Ptr{Cvoid},
               (Tke === Int64 ? 1 : 0)::Cint, length(plan.recv_rank_ids)::Cint,
               Int32.(plan.recv_rank_ids)::Ptr{Int32}, recv_counts::Ptr{Int64},
               width::Cint, 1::Cint)::Cint), "hpcla_halo_plan_create_ex")
        comm isa CommMPI && _attach_halo_window(_rccl(comm), halo[], comm.comm, nranks, (n_own, segments))
        interior, boundary = _classify_blocks(A, rp0, colval_split, n_own, rpb)
        # the ghost buffer of a single-buffered plan is a constant: fetched once, at plan time
        ghost = Ref{Ptr{Cvoid}}(C_NULL); ng = Ref{Int64}(0)
        _check(@ccall(LIB.hpcla_halo_ghost_ptr(halo[]::Ptr{Cvoid}, ghost::Ptr{Ptr{Cvoid}}, ng::Ptr{Int64})::Cint), "hpcla_halo_ghost_ptr")
        (halo[], interior, boundary, send_idx, ghost[], colval_split, rp0)
    end
end

# RUN TILES (k = 16; csrc/spmm.hip): for banded / stencil matrices the 64 rows of an SpMM row block touch a few contiguous
# runs of B rows; their descriptors are built once per plan (hpcla_spmm_runs_build_*) and the product then stages the
# runs' rows into LDS instead of gathering a row per stored entry (5-point matrix x 16: 0.47 ms against 0.52, same bits).
# Used when (nearly) all blocks fit; unstructured matrices keep the gather kernel.
const _spmm_runs_cache = IdDict{Any,Any}()     # device plan -> (run descriptors::ROCVector{UInt8}, banded::Bool)
function _spmm_runs_info(A, d::ROCVectorPlan{Tk}) where {Tk}
    get!(_spmm_runs_cache, d) do
        desc = AMDGPU.zeros(UInt8, @ccall LIB.hpcla_spmm_runs_desc_bytes(A.nrows_local::Int64)::Int64)
        nfit = Ref{Int64}(0); nnz = length(A.nzval)
        if Tk === Int32
            _check(@ccall(LIB.hpcla_spmm_runs_build_i32(_ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
                   A.nrows_local::Int64, nnz::Int64, 0::Cint, d.n_own::Int64, _ptr(desc)::Ptr{Cvoid}, nfit::Ptr{Int64},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_runs_build_i32")
        else
            _check(@ccall(LIB.hpcla_spmm_runs_build_i64(_ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
                   A.nrows_local::Int64, nnz::Int64, 0::Cint, d.n_own::Int64, _ptr(desc)::Ptr{Cvoid}, nfit::Ptr{Int64},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_runs_build_i64")
        end
        (desc, nfit[] >= 0.99 * cld(A.nrows_local, 64))
    end
end
_spmm_runs(A, d) = get(ENV, "HPCLA_SPMM_RUNS", "1") == "0" ? nothing : ((desc, fits) = _spmm_runs_info(A, d); fits ? desc : nothing)
# BANDED structure (every stencil: the 5-point matrix has 3 runs per block, the 7-point one 5): (nearly) every 64-row block
# touches at most 16 contiguous runs of columns (hpcla_spmm_banded_blocks_*, one pass at plan time).  There the lanes = rows
# kernels read a column-major block -- Julia's Matrix -- in contiguous pieces, so A * B runs on the caller's arrays as they are
# (csrc/colmajor.hip: 0.67 ms on the 5-point matrix x 16 where the two layout conversions around the row-major product cost
# 1.52 ms; 7-point: 0.99 against 1.63); an unstructured matrix touches a line per (entry, column) pair in that layout and
# keeps the conversion of B.  HPCLA_SPMM_COLMAJOR=0 switches the direct path off.
# The verdict is COLLECTIVE (an all-reduce, once per plan): the two paths exchange ghost rows of different widths for an odd
# k (k, or the padded pitch k + 1), so every rank of the communicator must take the same one.
const _banded_cache = IdDict{Any,Bool}()       # device plan -> banded on every rank?
const _spmm_cm_tuned = IdDict{Any,Int}()       # device plan -> block-order group measured for the column-major run tiles
# The library keeps ONE SpMM block order per rowptr array (hpcla_spmm_block_order_hint) while the orders are measured per
# KERNEL: the column-major run tiles (k = 16) have a measured group, every other SpMM launch of this file runs in the natural
# order.  Before a launch, the order IT wants is put in force if the last launch over the same rowptr left another one
# (the twin of dense.py _spmm_apply_order).  Every order is a bijection of the row blocks: results never depend on it.
const _spmm_order_in_force = IdDict{Any,Int}() # rowptr array -> group the library holds for it (1 = natural)
function _spmm_order!(rp0, group::Int)
    get(_spmm_order_in_force, rp0, 1) == group && return
    @ccall LIB.hpcla_spmm_block_order_hint(_ptr(rp0)::Ptr{Cvoid}, (group <= 1 ? 0 : group)::Cint)::Cint
    _spmm_order_in_force[rp0] = group
    return
end
function _banded(A, d::ROCVectorPlan{Tk}) where {Tk}
    get!(_banded_cache, d) do
        nb = Ref{Int64}(0); nnz = length(A.nzval)
        if get(ENV, "HPCLA_SPMM_COLMAJOR", "1") == "0"
            nb[] = -1                                        # (still takes part in the all-reduce below)
        elseif Tk === Int32
            _check(@ccall(LIB.hpcla_spmm_banded_blocks_i32(_ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
                   A.nrows_local::Int64, nnz::Int64, 0::Cint, d.n_own::Int64, 16::Cint, nb::Ptr{Int64},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_banded_blocks_i32")
        else
            _check(@ccall(LIB.hpcla_spmm_banded_blocks_i64(_ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
                   A.nrows_local::Int64, nnz::Int64, 0::Cint, d.n_own::Int64, 16::Cint, nb::Ptr{Int64},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_banded_blocks_i64")
        end
        mine = nb[] >= 0.99 * cld(A.nrows_local, 64) ? 1 : 0
        HPCLinearAlgebra.comm_allreduce(A.backend.comm, mine, min) == 1
    end
end

# A * B on the column-major blocks themselves (T = Float64 or Float32): without neighbours one launch; with neighbours the
# exchange is posted from the column-major block (hpcla_halo_begin_strided_*: the rows the plan sends are staged row-major,
# Float32 values widened), interior 256-row blocks overlap it, boundary blocks read the plan's row-major ghost segment.
function _spmm_colmajor(A::HPCSparseMatrix{T,Ti,B}, M::HPCMatrix{T,B}, plan, d::ROCVectorPlan{Tk}) where {T<:Union{Float32,Float64},Ti,Tk,B<:ROCBackend}
    nloc, k = size(M.A)
    C = ROCMatrix{T}(undef, A.nrows_local, k)          # every row block is launched: no zero fill
    nnz = length(A.nzval); ldb = max(nloc, 1); ldc = max(A.nrows_local, 1)
    nranks = comm_size(A.backend.comm)
    # (whole slices -- small matrices: a banded structure asks for a few rows per neighbour -- move the ghost positions: the run
    # descriptors describe the vector plan's columns and stay out then)
    own_lists = nranks == 1 || !any(==(1), _whole_slice_wishes(plan, M.row_partition, nranks))
    # k = 16, Float64, every block within the run-tile limits (a 5-point matrix: 3 runs per block) and B's columns on the
    # 16-byte grid: the run tiles on the column-major blocks (hpcla_spmm_runs_colmajor_k16_f64_*, round 5: 0.56 ms against
    # 0.64 on the 5-point matrix x 16, same bits) -- block lists over its 64-row blocks
    runs = (T === Float64 && k == 16 && own_lists && iseven(ldb) && UInt(_ptr(M.A)) % 16 == 0) ? _spmm_runs(A, d) : nothing
    rpb = runs === nothing ? (@ccall LIB.hpcla_spmv_rows_per_block()::Cint) : (@ccall LIB.hpcla_spmm_rows_per_block()::Cint)
    # every rank of a communicator takes part in the plan-time collectives of the exchange entry, neighbours or not
    ent = nranks > 1 ? _spmm_halo(A, plan, d, M.row_partition, k, rpb) : (C_NULL, nothing, nothing, nothing, C_NULL, d.colval_split, d.rowptr0)
    halo, interior, boundary, _, ghost_seg, colval_split, rp0 = ent
    Te = eltype(rp0)                                   # index type of the entry's kernel arrays
    # PLAN TIME, once per device plan: the block order of the run tiles BY MEASUREMENT (the same launch timed under five block
    # orders, the fastest stays set) -- over every block, or over the interior list of a rank with neighbours; BEFORE any exchange
    # is posted, so that nothing else is in flight while it is timed (the timed launches write those rows of C, correctly)
    if runs !== nothing && !haskey(_spmm_cm_tuned, d)
        tb = halo == C_NULL ? nothing : interior
        chosen = Ref{Cint}(1)
        if tb !== nothing && isempty(tb)
            # (nothing to time without an interior block)
        elseif Te === Int32
            _check(@ccall(LIB.hpcla_spmm_runs_colmajor_tune_block_order_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, C_NULL::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                   _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(runs)::Ptr{Cvoid},
                   _ptr(tb)::Ptr{Cvoid}, _len(tb)::Int64, _stream()::Ptr{Cvoid}, chosen::Ptr{Cint})::Cint),
                   "hpcla_spmm_runs_colmajor_tune_block_order_f64_i32")
        else
            _check(@ccall(LIB.hpcla_spmm_runs_colmajor_tune_block_order_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, C_NULL::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                   _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(runs)::Ptr{Cvoid},
                   _ptr(tb)::Ptr{Cvoid}, _len(tb)::Int64, _stream()::Ptr{Cvoid}, chosen::Ptr{Cint})::Cint),
                   "hpcla_spmm_runs_colmajor_tune_block_order_f64_i64")
        end
        _spmm_cm_tuned[d] = Int(chosen[]); _spmm_order_in_force[rp0] = Int(chosen[])      # (what the tuner left set)
    end
    function launch(ghost::Ptr{Cvoid}, blocks::Ptr{Cvoid}, nblocks::Int64)
        if runs !== nothing
            _spmm_order!(rp0, get(_spmm_cm_tuned, d, 1))
            if Te === Int32
                _check(@ccall(LIB.hpcla_spmm_runs_colmajor_k16_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                       _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                       _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(runs)::Ptr{Cvoid},
                       blocks::Ptr{Cvoid}, nblocks::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_runs_colmajor_k16_f64_i32")
            else
                _check(@ccall(LIB.hpcla_spmm_runs_colmajor_k16_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                       _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                       _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(runs)::Ptr{Cvoid},
                       blocks::Ptr{Cvoid}, nblocks::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_runs_colmajor_k16_f64_i64")
            end
        elseif T === Float64 && Te === Int32
            _check(@ccall(LIB.hpcla_spmm_split_colmajor_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                   _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint, blocks::Ptr{Cvoid},
                   nblocks::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_colmajor_f64_i32")
        elseif T === Float64
            _check(@ccall(LIB.hpcla_spmm_split_colmajor_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                   _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint, blocks::Ptr{Cvoid},
                   nblocks::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_colmajor_f64_i64")
        elseif Te === Int32
            _check(@ccall(LIB.hpcla_spmm_split_colmajor_f32_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                   _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint, blocks::Ptr{Cvoid},
                   nblocks::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_colmajor_f32_i32")
        else
            _check(@ccall(LIB.hpcla_spmm_split_colmajor_f32_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, k::Int64, d.n_own::Int64,
                   _ptr(C)::Ptr{Cvoid}, ldc::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint, blocks::Ptr{Cvoid},
                   nblocks::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_colmajor_f32_i64")
        end
    end
    if halo == C_NULL
        launch(C_NULL, C_NULL, Int64(0))                         # every row block, every column owned
    else
        stage = _stage(d, d.n_own * k)
        if T === Float64
            _check(@ccall(LIB.hpcla_halo_begin_strided_f64(halo::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, 1::Int64, ldb::Int64,
                   _ptr(stage)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_begin_strided_f64")
        else
            _check(@ccall(LIB.hpcla_halo_begin_strided_f32(halo::Ptr{Cvoid}, _ptr(M.A)::Ptr{Cvoid}, 1::Int64, ldb::Int64,
                   _ptr(stage)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_begin_strided_f32")
        end
        isempty(interior) || launch(C_NULL, _ptr(interior), Int64(length(interior)))     # overlaps the exchange
        _check(@ccall(LIB.hpcla_halo_end(halo::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_end")
        isempty(boundary) || launch(ghost_seg, _ptr(boundary), Int64(length(boundary)))
    end
    return _spmm_result(A, C, k)
end

# Row-major B rows (own block `Brow`, ghost segment `ghost`, both on the row pitch `ldb`) times A into C, over the kernel arrays
# `rp0` / `colval_split` of the exchange entry.  `blocks` = nothing: every row block (no list is built or uploaded).
# `ccol` = false: `C` is row-major on the pitch `ldb` (k x nrows column-major storage when ldb == k), run tiles where the
# structure allows them (`runs`); `ccol` = true (round 5): `C` is the caller's column-major nrows x k Matrix and the product
# stores it in that layout itself (hpcla_spmm_split_ccol_f64_*, csrc/spmm.hip CCOL) -- no conversion of C afterwards.
# ODD k (round 6): ldb = k + 1 -- the vector kernel owns column pairs and reads the padding double of every row it gathers.
function _spmm_split!(C, A::HPCSparseMatrix{T,Ti,B}, rp0, colval_split, n_own::Int, Brow, ldb::Int, ghost::Ptr{Cvoid}, k::Int, blocks,
                      ccol::Bool, runs=nothing) where {T,Ti,B}
    blocks !== nothing && isempty(blocks) && return
    nnz = length(A.nzval); nb = _len(blocks)
    _spmm_order!(rp0, 1)                               # the gather kernel's launches of this file: the natural order
    if ccol && eltype(rp0) === Int32
        _check(@ccall(LIB.hpcla_spmm_split_ccol_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, ldb::Int64, n_own::Int64,
               _ptr(C)::Ptr{Cvoid}, max(A.nrows_local, 1)::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint,
               _ptr(blocks)::Ptr{Cvoid}, nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_ccol_f64_i32")
    elseif ccol
        _check(@ccall(LIB.hpcla_spmm_split_ccol_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, ldb::Int64, n_own::Int64,
               _ptr(C)::Ptr{Cvoid}, max(A.nrows_local, 1)::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint,
               _ptr(blocks)::Ptr{Cvoid}, nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_ccol_f64_i64")
    elseif runs !== nothing && eltype(rp0) === Int32
        _check(@ccall(LIB.hpcla_spmm_runs_k16_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, ghost::Ptr{Cvoid}, n_own::Int64, _ptr(C)::Ptr{Cvoid},
               A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(runs)::Ptr{Cvoid}, _ptr(blocks)::Ptr{Cvoid},
               nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_runs_k16_f64_i32")
    elseif runs !== nothing
        _check(@ccall(LIB.hpcla_spmm_runs_k16_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, ghost::Ptr{Cvoid}, n_own::Int64, _ptr(C)::Ptr{Cvoid},
               A.nrows_local::Int64, nnz::Int64, 0::Cint, _ptr(runs)::Ptr{Cvoid}, _ptr(blocks)::Ptr{Cvoid},
               nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_runs_k16_f64_i64")
    elseif eltype(rp0) === Int32
        _check(@ccall(LIB.hpcla_spmm_split_f64_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, ldb::Int64, n_own::Int64,
               _ptr(C)::Ptr{Cvoid}, ldb::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint,
               _ptr(blocks)::Ptr{Cvoid}, nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_f64_i32")
    else
        _check(@ccall(LIB.hpcla_spmm_split_f64_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, ldb::Int64, ghost::Ptr{Cvoid}, ldb::Int64, n_own::Int64,
               _ptr(C)::Ptr{Cvoid}, ldb::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint,
               _ptr(blocks)::Ptr{Cvoid}, nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_f64_i64")
    end
end

function Base.:*(A::HPCSparseMatrix{T,Ti,B}, M::HPCMatrix{T,B}) where {T<:Float64,Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, M.backend)
    nloc, k = size(M.A)
    plan, d = _spmm_vector_plan(A, M)
    k > 1 && _banded(A, d) && return _spmm_colmajor(A, M, plan, d)       # banded structure: no layout conversion at all
    # UNSTRUCTURED: B converted once to row-major rows (an unstructured matrix gathers whole B rows: one 128-byte line per
    # stored entry at k = 16); C comes out of the product column-major (round 5: no second conversion -- config 5 through
    # this path 2.25 -> 2.12 ms at N = 1 where the B conversion of all 2^24 rows costs 0.75 of them; at 8 GPUs a rank
    # converts its own 2^21 rows, 0.09 ms).  The rows sit on an EVEN pitch (round 6): kp = k + 1 for an odd k, whose products
    # then take the vector kernel (5-point matrix x 15: 0.946 ms on the one-column-per-lane kernel against 0.475 for 16);
    # ghost rows travel on the same pitch.  Any k: the library tiles a column-major C wider than 16 columns.
    kp = k + (k & 1)
    Brow = ROCMatrix{T}(undef, kp, nloc)            # kp x nloc column-major == nloc rows of pitch kp (the transpose writes columns 1:k)
    _check(@ccall(LIB.hpcla_transpose_f64(_ptr(M.A)::Ptr{Cvoid}, max(nloc, 1)::Int64, 1::Cint, _ptr(Brow)::Ptr{Cvoid}, kp::Int64,
           0::Cint, nloc::Int64, k::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_transpose_f64")
    C = ROCMatrix{T}(undef, A.nrows_local, k)       # every row block is launched: no zero fill
    if comm_size(A.backend.comm) == 1
        _spmm_split!(C, A, d.rowptr0, d.colval_split, d.n_own, Brow, kp, C_NULL, k, nothing, true)
    else
        # (every rank, with or without neighbours: the entry's first use is collective)
        halo, interior, boundary, _, ghost, colval_split, rp0 =
            _spmm_halo(A, plan, d, M.row_partition, kp, (@ccall LIB.hpcla_spmm_rows_per_block()::Cint))
        if halo == C_NULL
            _spmm_split!(C, A, rp0, colval_split, d.n_own, Brow, kp, C_NULL, k, nothing, true)
        else
            _check(@ccall(LIB.hpcla_halo_begin(halo::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_begin")
            _spmm_split!(C, A, rp0, colval_split, d.n_own, Brow, kp, ghost, k, interior, true)   # rows without ghost columns overlap the exchange
            _check(@ccall(LIB.hpcla_halo_end(halo::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_end")
            _spmm_split!(C, A, rp0, colval_split, d.n_own, Brow, kp, ghost, k, boundary, true)   # ghost rows arrived row-major: nothing else is converted
        end
    end
    return _spmm_result(A, C, k)
end

# ==== structural hash without the host pass over colval  (replaces the local Blake3 pass of compute_structural_hash,
# src/sparse.jl:97-121, for DeviceROCm matrices; SURVEY 8 a6) ===============================================================
# The reference hashes row_partition, col_indices, rowptr and colval on the host -- at config 3 that is 335 MB of colval per
# rank read on first use.  colval already lives on the device (colval_target): hpcla_digest_* reduces it there to four 64-bit
# order-sensitive words (csrc/construct.hip digest_kernel), and those words stand in for its bytes in the rank-local hash; the
# Allgather of the local hashes and the hash of hashes are the reference's.  A memoization key only (compared for equality):
# all ranks take this method together, so the key is uniform across ranks like the reference's.  Other index types: parent.
function HPCLinearAlgebra._ensure_hash(A::HPCSparseMatrix{T,Ti,B}) where {T,Ti,B<:ROCBackend}
    A.structural_hash === nothing || return A.structural_hash
    (Ti === Int32 || Ti === Int64) && A.colval_target isa ROCVector ||
        return invoke(HPCLinearAlgebra._ensure_hash, Tuple{HPCSparseMatrix}, A)
    words = zeros(UInt64, 4); n = length(A.colval_target)
    if Ti === Int32
        _check(@ccall(LIB.hpcla_digest_i32(_ptr(A.colval_target)::Ptr{Cvoid}, n::Int64, words::Ptr{UInt64}, _stream()::Ptr{Cvoid})::Cint),
               "hpcla_digest_i32")
    else
        _check(@ccall(LIB.hpcla_digest_i64(_ptr(A.colval_target)::Ptr{Cvoid}, n::Int64, words::Ptr{UInt64}, _stream()::Ptr{Cvoid})::Cint),
               "hpcla_digest_i64")
    end
    ctx = HPCLinearAlgebra.Blake3Ctx()                      # length-prefixed pieces, as src/sparse.jl:103-111
    for piece in (A.row_partition, A.col_indices, A.rowptr)
        HPCLinearAlgebra.update!(ctx, reinterpret(UInt8, Int[length(piece)]))
        HPCLinearAlgebra.update!(ctx, reinterpret(UInt8, piece))
    end
    HPCLinearAlgebra.update!(ctx, reinterpret(UInt8, Int[n]))
    HPCLinearAlgebra.update!(ctx, reinterpret(UInt8, words))
    all_hashes = HPCLinearAlgebra.comm_allgather(A.backend.comm, HPCLinearAlgebra.digest(ctx))
    ctx2 = HPCLinearAlgebra.Blake3Ctx()
    HPCLinearAlgebra.update!(ctx2, reduce(vcat, all_hashes))
    A.structural_hash = HPCLinearAlgebra.Blake3Hash(HPCLinearAlgebra.digest(ctx2))
    return A.structural_hash
end

# ==== HPCSparseMatrix_local on the device  (SURVEY 8f rank 2; replaces `unique!(sort(copy(rowval)))` + one binary search per
# stored entry, src/sparse.jl:501-509, 137-144) ============================================================================
# The caller's rows arrive as CSR with GLOBAL columns (the parent's contract, :454-470).  The column compression -- which
# columns occur, and the local index of every entry -- runs on the device: presence bitmap over the rows' column window,
# exclusive scan, emit (hpcla_compress_columns_*, csrc/construct.hip): O(nnz + window) instead of O(nnz log nnz) on one host
# core; at 4 x 10^7 entries per rank the host version is seconds of the time to the first product.  Everything else is the
# parent's constructor, step by step: row partition from an Allgather of the local sizes, host copies of rowptr / colval /
# col_indices (the struct's "always CPU" fields), lazy structural hash.  Falls through to the parent when the column window is
# out of proportion to the entries (its scratch grows with the window), for empty matrices and for index types other than Int32 / Int64.
function HPCLinearAlgebra.HPCSparseMatrix_local(A_local::HPCLinearAlgebra.SparseMatrixCSR{T,Timat}, backend::B;
        col_partition::Vector{Int}=HPCLinearAlgebra.uniform_partition(A_local.parent.m, comm_size(backend.comm))) where {T,Timat,B<:ROCBackend}
    Ti = indextype_backend(backend)
    AT = A_local.parent                                     # CSC of the transpose: colptr = row pointers, rowval = global columns
    nnz = length(AT.rowval)
    parent_path() = invoke(HPCLinearAlgebra.HPCSparseMatrix_local, Tuple{HPCLinearAlgebra.SparseMatrixCSR{T,Timat},HPCBackend}, A_local, backend;
                           col_partition=col_partition)
    (nnz > 0 && (Ti === Int32 || Ti === Int64)) || return parent_path()
    lo, hi = extrema(AT.rowval)                             # one host pass; 1-based global columns
    window = Int64(hi - lo + 1)
    # the bitmap / scan scratch grows with the WINDOW, not with nnz: a few scattered columns over a huge range stay on the host
    window <= 64 * Int64(nnz) + (Int64(1) << 24) || return parent_path()
    work_bytes = @ccall LIB.hpcla_colspace_work_bytes(window::Int64)::Int64
    comm = backend.comm; nranks = comm_size(comm)
    all_info = reshape(HPCLinearAlgebra.comm_allgather(comm, Int32[AT.n, AT.m]), 2, nranks)
    all(c == all_info[2, 1] for c in all_info[2, :]) ||
        error("HPCSparseMatrix_local: All ranks must have the same number of columns. Got column counts: $(all_info[2, :])")
    row_partition = Vector{Int}(undef, nranks + 1); row_partition[1] = 1
    for r in 1:nranks; row_partition[r+1] = row_partition[r] + all_info[1, r]; end
    cols_dev = ROCVector(Int64.(AT.rowval) .- 1)            # 0-based global columns
    colval_target = ROCVector{Ti}(undef, nnz)
    ci_dev = ROCVector{Int64}(undef, window); work = ROCVector{UInt8}(undef, work_bytes)
    ncomp = Ref{Int64}(0)
    if Ti === Int32
        _check(@ccall(LIB.hpcla_compress_columns_i32(_ptr(cols_dev)::Ptr{Cvoid}, nnz::Int64, Int64(lo - 1)::Int64, window::Int64,
               _ptr(colval_target)::Ptr{Cvoid}, 1::Cint, _ptr(ci_dev)::Ptr{Cvoid}, ncomp::Ptr{Int64}, _ptr(work)::Ptr{Cvoid},
               _stream()::Ptr{Cvoid})::Cint), "hpcla_compress_columns_i32")
    else
        _check(@ccall(LIB.hpcla_compress_columns_i64(_ptr(cols_dev)::Ptr{Cvoid}, nnz::Int64, Int64(lo - 1)::Int64, window::Int64,
               _ptr(colval_target)::Ptr{Cvoid}, 1::Cint, _ptr(ci_dev)::Ptr{Cvoid}, ncomp::Ptr{Int64}, _ptr(work)::Ptr{Cvoid},
               _stream()::Ptr{Cvoid})::Cint), "hpcla_compress_columns_i64")
    end
    col_indices = Int.(Array(ci_dev[1:ncomp[]])) .+ 1       # ascending global columns, 1-based (src/sparse.jl:501)
    rowptr = convert(Vector{Ti}, AT.colptr)
    colval = Array(colval_target)                           # the struct's host copy (compress_AT's rowval, :137-144)
    nzval = HPCLinearAlgebra._convert_array(AT.nzval, backend.device)
    rowptr_target = HPCLinearAlgebra._to_target_device(rowptr, backend.device)
    return HPCSparseMatrix{T,Ti,B}(nothing, row_partition, col_partition, col_indices, rowptr, colval, nzval, AT.n, length(col_indices),
                                   nothing, nothing, rowptr_target, colval_target, backend)
end

# ==== A[rows, cols] and A[:, k] on the device  (replace the host walks over `_get_csc(A)` of src/indexing.jl:691-840, 872-914) ==
# The parent counts, collects, sorts and recompresses the kept entries one by one on the host (:775-819) and scans every row
# for column k (:891-908): on a device backend that is scalar indexing of device arrays or a round trip of the matrix.  Here:
# col_indices is sorted, so the column range is ONE window [j0, j1) of compressed local columns (two binary searches on the
# host); columns ascend within a row (src/sparse.jl:288-295), so a row keeps ONE contiguous run.  hpcla_submatrix_structure_*
# locates the runs, scans the counts into the new rowptr and a presence bitmap into the column look-up table; one coalesced
# hpcla_submatrix_fill_* copies nzval and writes the recompressed colval (csrc/submatrix.hip).  No communication, as in the
# parent: the row partition is _compute_subpartition's.  The values never leave the device; the struct's host fields (rowptr,
# colval, col_indices: "always CPU") come back once per call -- that is the struct's contract, not staging of the values.
# The parent's `:` convenience methods (:843-855) land on the first method.  Empty and out-of-bounds ranges, and index types
# other than Int32 / Int64, are the parent's (its empty matrix has a uniform row partition, :709-724).
# Mirrors linearalgebrampi.jl_amd/indexing.py, which the GPU tests hold to a numpy restatement bit for bit.
const _MovedBits = Union{Float32,Float64}         # the kernels move values by size (4 or 8 bytes) and never compute with them
function Base.getindex(A::HPCSparseMatrix{T,Ti,B}, row_rng::UnitRange{Int}, col_rng::UnitRange{Int}) where {T<:_MovedBits,Ti<:Union{Int32,Int64},B<:ROCBackend}
    m, n = size(A)
    (first(row_rng) < 1 || last(row_rng) > m || first(col_rng) < 1 || last(col_rng) > n || isempty(row_rng) || isempty(col_rng)) &&
        return invoke(Base.getindex, Tuple{HPCSparseMatrix,UnitRange{Int},UnitRange{Int}}, A, row_rng, col_rng)   # PCIe: none -- the parent's error, or its empty matrix (src/indexing.jl:709-724): no stored entry is involved
    comm = A.backend.comm; rank = comm_rank(comm); nranks = comm_size(comm)
    new_row_partition = HPCLinearAlgebra._compute_subpartition(A.row_partition, row_rng)
    new_col_partition = HPCLinearAlgebra.uniform_partition(length(col_rng), nranks)
    my_start = A.row_partition[rank+1]
    lo = max(my_start, first(row_rng)); hi = min(A.row_partition[rank+2] - 1, last(row_rng))
    r0 = lo <= hi ? lo - my_start : 0                       # this rank's rows of the range: local, 0-based, half-open [r0, r1)
    r1 = lo <= hi ? hi - my_start + 1 : 0
    j0 = searchsortedfirst(A.col_indices, first(col_rng)) - 1          # compressed local columns [j0, j1), 0-based
    j1 = searchsortedfirst(A.col_indices, last(col_rng) + 1) - 1
    nsel = r1 - r0; width = j1 - j0; nnz = length(A.nzval); eb = Cint(T === Float64 ? 8 : 4)
    work = ROCVector{UInt8}(undef, @ccall LIB.hpcla_submatrix_work_bytes(nsel::Int64, width::Int64)::Int64)
    src_start = ROCVector{Int64}(undef, nsel); rowptr_target = ROCVector{Ti}(undef, nsel + 1)
    kept_dev = ROCVector{Int64}(undef, width)
    new_nnz = Ref{Int64}(0); ncomp = Ref{Int64}(0)
    # rowptr_target / colval_target are 1-based (index_base = 1); col_indices_src = NULL: the kept LOCAL columns come back
    if Ti === Int32
        _check(@ccall(LIB.hpcla_submatrix_structure_i32(_ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid},
               A.nrows_local::Int64, nnz::Int64, r0::Int64, r1::Int64, j0::Int64, j1::Int64, 1::Cint, C_NULL::Ptr{Cvoid}, 0::Int64,
               _ptr(src_start)::Ptr{Cvoid}, _ptr(rowptr_target)::Ptr{Cvoid}, _ptr(kept_dev)::Ptr{Cvoid}, new_nnz::Ptr{Int64},
               ncomp::Ptr{Int64}, _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_submatrix_structure_i32")
    else
        _check(@ccall(LIB.hpcla_submatrix_structure_i64(_ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid},
               A.nrows_local::Int64, nnz::Int64, r0::Int64, r1::Int64, j0::Int64, j1::Int64, 1::Cint, C_NULL::Ptr{Cvoid}, 0::Int64,
               _ptr(src_start)::Ptr{Cvoid}, _ptr(rowptr_target)::Ptr{Cvoid}, _ptr(kept_dev)::Ptr{Cvoid}, new_nnz::Ptr{Int64},
               ncomp::Ptr{Int64}, _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_submatrix_structure_i64")
    end
    colval_target = ROCVector{Ti}(undef, new_nnz[]); nzval = similar(A.nzval, new_nnz[])
    if Ti === Int32
        _check(@ccall(LIB.hpcla_submatrix_fill_i32(eb::Cint, _ptr(A.colval_target)::Ptr{Cvoid}, _ptr(A.nzval)::Ptr{Cvoid}, nnz::Int64,
               _ptr(src_start)::Ptr{Cvoid}, _ptr(rowptr_target)::Ptr{Cvoid}, nsel::Int64, new_nnz[]::Int64, j0::Int64, j1::Int64,
               1::Cint, _ptr(work)::Ptr{Cvoid}, _ptr(colval_target)::Ptr{Cvoid}, _ptr(nzval)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint),
               "hpcla_submatrix_fill_i32")
    else
        _check(@ccall(LIB.hpcla_submatrix_fill_i64(eb::Cint, _ptr(A.colval_target)::Ptr{Cvoid}, _ptr(A.nzval)::Ptr{Cvoid}, nnz::Int64,
               _ptr(src_start)::Ptr{Cvoid}, _ptr(rowptr_target)::Ptr{Cvoid}, nsel::Int64, new_nnz[]::Int64, j0::Int64, j1::Int64,
               1::Cint, _ptr(work)::Ptr{Cvoid}, _ptr(colval_target)::Ptr{Cvoid}, _ptr(nzval)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint),
               "hpcla_submatrix_fill_i64")
    end
    kept = Array(kept_dev[1:ncomp[]])                       # PCIe: 8 B per kept column -- the struct's host col_indices (which local columns occur)
    col_indices = A.col_indices[kept .+ 1] .- (first(col_rng) - 1)     # global columns of the result, 1-based, ascending (:807-819)
    rowptr = Array(rowptr_target)                           # PCIe: (rows + 1) index words -- the struct's host rowptr ("always CPU")
    colval = Array(colval_target)                           # PCIe: one index word per kept entry -- the struct's host colval; nzval stays on the device
    return HPCSparseMatrix{T,Ti,B}(nothing, new_row_partition, new_col_partition, col_indices, rowptr, colval, nzval, nsel, length(col_indices),
                                   nothing, nothing, rowptr_target, colval_target, A.backend)
end

function Base.getindex(A::HPCSparseMatrix{T,Ti,B}, ::Colon, k::Integer) where {T<:_MovedBits,Ti<:Union{Int32,Int64},B<:ROCBackend}
    m, n = size(A)
    (k < 1 || k > n) && error("HPCSparseMatrix column index out of bounds: k=$k, ncols=$n")
    jk = searchsortedfirst(A.col_indices, k)                # 1-based local column, if this rank stores column k at all
    has_col = jk <= length(A.col_indices) && A.col_indices[jk] == k
    # not stored on this rank: all zeros, no kernel (:888-894); else one look-up per row writes every element
    out = (has_col && A.nrows_local > 0) ? similar(A.nzval, A.nrows_local) : AMDGPU.zeros(T, A.nrows_local)
    if has_col && A.nrows_local > 0
        nnz = length(A.nzval); eb = Cint(T === Float64 ? 8 : 4)
        if Ti === Int32
            _check(@ccall(LIB.hpcla_sparse_column_i32(eb::Cint, _ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, A.nrows_local::Int64, nnz::Int64, (jk - 1)::Int64, 1::Cint, _ptr(out)::Ptr{Cvoid},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_sparse_column_i32")
        else
            _check(@ccall(LIB.hpcla_sparse_column_i64(eb::Cint, _ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, A.nrows_local::Int64, nnz::Int64, (jk - 1)::Int64, 1::Cint, _ptr(out)::Ptr{Cvoid},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_sparse_column_i64")
        end
    end
    return HPCVector{T,B}(_partition_hash(A.row_partition), copy(A.row_partition), out, A.backend)
end

# ==== sparse A * B  (SURVEY 8f rank 3; replaces the CPU SparseArrays multiply inside src/sparse.jl:991-1059) ===============
# The parent's memoized MatrixPlan (src/sparse.jl:554-978) keeps gathering the rows of B that A.col_indices names; its
# execute_plan! takes a device target (:917-975), so the gathered values are written into device memory.  What changes is the
# LOCAL product: `CT = plan.AT * A_csc` (:1011 -- on the CPU for GPU backends too) becomes hpcla_spgemm_ub / _numeric /
# _compact on the device (csrc/spgemm.hip: Gustavson per row, k ascending, so every C(i, j) is summed in the reference's
# order), and the result's column space is compressed on the device.  From the third product on a structure the per-entry
# product lists are built once (host, plan time) and the numeric product is one streaming pass (hpcla_spgemm_numeric_mapped_f64).
# Mirrors linearalgebrampi.jl_amd/matmat.py, which is executed and held to the oracle's bits by the GPU tests.  Falls through
# to the parent -- all ranks together -- when an output row has more candidate entries than the largest bin handles, and for
# index types other than Int32 / Int64.
mutable struct ROCSpgemmState
    g_rowptr::Any            # ROCVector{Int64}: row pointers of the gathered rows G, 0-based
    g_col::Any               # ROCVector{Int64}: G's GLOBAL columns, 0-based
    bins::Vector{Any}        # (bin::Cint, rows::ROCVector{Int32}): output rows by candidate count
    ub_prefix::Any           # ROCVector{Int64}: slots of the first product (upper bounds); nothing afterwards
    total_ub::Int64
    cnt::Any                 # ROCVector{Int64}: entries per output row
    result::Any              # nothing | NamedTuple (structure of C, kept for repeated products)
    repeats::Int
    map::Any                 # nothing: not tried | :none: not built | (pair_ptr, pairs, ptr_is_i64)
end
const _spgemm_cache = IdDict{Any,Any}()    # reference MatrixPlan -> ROCSpgemmState | nothing (parent path)
# What a state pins until clear_rocm_plan_cache!: the gathered rows' structure (g_rowptr, g_col), the bins, the result's
# STRUCTURE -- and, the large part, the per-entry product lists (8 B per product, up to HPCLA_SPGEMM_MAP_MAX = 5e7 products =
# 400 MB per structure).  The lists are bounded across structures: at most HPCLA_SPGEMM_MAP_KEEP (default 4) states hold
# them, least recently multiplied first out -- an evicted structure goes back to the numeric kernels (same bits) and
# rebuilds its lists if it is multiplied three more times.
# The result matrices of one structure SHARE their structure arrays (col_indices, colptr / rowptr, colval and the device copies):
# the parent treats those fields as immutable after construction (every operator builds new arrays, none writes into an
# operand's), and its own cached plans alias structure the same way (AdditionPlan results, cached_transpose); only nzval is
# fresh per product.  A caller that mutates a result's structure in place must copy it first.
const _spgemm_map_lru = Any[]              # states holding product lists, least recently used first
function _spgemm_touch_lists!(st)
    filter!(s -> s !== st, _spgemm_map_lru); push!(_spgemm_map_lru, st)
    keep = max(1, parse(Int, get(ENV, "HPCLA_SPGEMM_MAP_KEEP", "4")))
    while length(_spgemm_map_lru) > keep
        old = popfirst!(_spgemm_map_lru)
        old.map = nothing; old.repeats = 0                 # lists released; the numeric kernels take over (same bits)
    end
    return
end

function _spgemm_symbolic(A::HPCSparseMatrix{T,Ti,B}, plan) where {T,Ti,B}
    nrows = A.nrows_local
    g_rowptr = ROCVector(Int64.(plan.AT.colptr) .- 1)
    g_col = ROCVector(Int64.(plan.AT.rowval) .- 1)
    ub = AMDGPU.zeros(Int64, max(nrows, 1))
    if Ti === Int32
        _check(@ccall(LIB.hpcla_spgemm_ub_i32(_ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid}, nrows::Int64,
               1::Cint, _ptr(g_rowptr)::Ptr{Cvoid}, _ptr(ub)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_spgemm_ub_i32")
    else
        _check(@ccall(LIB.hpcla_spgemm_ub_i64(_ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid}, nrows::Int64,
               1::Cint, _ptr(g_rowptr)::Ptr{Cvoid}, _ptr(ub)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_spgemm_ub_i64")
    end
    ub_h = Array(ub)[1:nrows]
    caps = Int64[]
    while true                                              # the bins are the library's to define
        c = @ccall LIB.hpcla_spgemm_bin_cap(length(caps)::Cint)::Int64
        c < 0 && break
        push!(caps, c)
    end
    # the limit is checked COLLECTIVELY: every rank learns the worst row of any rank, all take the same path
    worst = HPCLinearAlgebra.comm_allreduce(A.backend.comm, isempty(ub_h) ? Int64(0) : maximum(ub_h), max)
    worst > caps[end] && return nothing
    bins = Any[]; lo = Int64(-1)
    for (b, cap) in enumerate(caps)
        rows = Int32.(findall(u -> lo < u <= cap, ub_h) .- 1)
        lo = cap
        isempty(rows) || push!(bins, (Cint(b - 1), ROCVector(rows)))
    end
    ub_prefix_h = vcat(Int64[0], cumsum(ub_h))
    return ROCSpgemmState(g_rowptr, g_col, bins, ROCVector(ub_prefix_h), ub_prefix_h[end], AMDGPU.zeros(Int64, max(nrows, 1)),
                          nothing, 0, nothing)
end

function _spgemm_numeric!(st::ROCSpgemmState, A::HPCSparseMatrix{T,Ti,B}, gval, offsets, col_out, val_out) where {T,Ti,B}
    for (b, rows) in st.bins
        if Ti === Int32
            _check(@ccall(LIB.hpcla_spgemm_numeric_i32(b::Cint, _ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, 1::Cint, _ptr(st.g_rowptr)::Ptr{Cvoid}, _ptr(st.g_col)::Ptr{Cvoid}, _ptr(gval)::Ptr{Cvoid},
                   _ptr(rows)::Ptr{Cvoid}, length(rows)::Int64, _ptr(offsets)::Ptr{Cvoid}, _ptr(col_out)::Ptr{Cvoid},
                   _ptr(val_out)::Ptr{Cvoid}, _ptr(st.cnt)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_spgemm_numeric_i32")
        else
            _check(@ccall(LIB.hpcla_spgemm_numeric_i64(b::Cint, _ptr(A.rowptr_target)::Ptr{Cvoid}, _ptr(A.colval_target)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, 1::Cint, _ptr(st.g_rowptr)::Ptr{Cvoid}, _ptr(st.g_col)::Ptr{Cvoid}, _ptr(gval)::Ptr{Cvoid},
                   _ptr(rows)::Ptr{Cvoid}, length(rows)::Int64, _ptr(offsets)::Ptr{Cvoid}, _ptr(col_out)::Ptr{Cvoid},
                   _ptr(val_out)::Ptr{Cvoid}, _ptr(st.cnt)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_spgemm_numeric_i64")
        end
    end
end

# Per result entry the list of its products as (index into A.nzval, index into the gathered values), 0-based, in ascending A
# entry (= ascending k: the order the numeric kernels add in).  Host, once per structure: expand every A entry over its G row,
# stable sort by (row, result column), run lengths.  Returns nothing when the lists would exceed `max_products` or Int32.
function _spgemm_product_lists(A::HPCSparseMatrix{T,Ti,B}, plan, res, max_products::Int) where {T,Ti,B}
    g_rp = Int64.(plan.AT.colptr); g_cl = Int64.(plan.AT.rowval)           # 1-based
    lens = [g_rp[k+1] - g_rp[k] for k in A.colval]                        # A.colval: 1-based rows of G
    total = sum(lens)
    (total == 0 || total > max_products || total > typemax(Int32) || length(g_cl) > typemax(Int32)) && return nothing
    ai = Vector{Int32}(undef, total); gi = Vector{Int32}(undef, total); key = Vector{Int64}(undef, total)
    width = Int64(max(maximum(g_cl), maximum(res.c_col_h)) + 1)
    t = 0
    for r in 1:A.nrows_local, e in A.rowptr[r]:(A.rowptr[r+1]-1)
        k = A.colval[e]
        for g in g_rp[k]:(g_rp[k+1]-1)
            t += 1
            ai[t] = e - 1; gi[t] = g - 1; key[t] = Int64(r) * width + (g_cl[g] - 1)       # 0-based column, like res.c_col_h
        end
    end
    perm = sortperm(key; alg=MergeSort)                                    # stable: products of one entry stay in ascending k
    ptr = zeros(Int64, res.nnz + 1)
    e = 0; last = Int64(-1)
    for i in perm
        if key[i] != last
            e += 1; last = key[i]
            e <= res.nnz || return nothing
            key[i] == Int64(res.c_row_h[e]) * width + res.c_col_h[e] || return nothing     # safety net: must reproduce C's structure
        end
        ptr[e+1] += 1
    end
    e == res.nnz || return nothing
    cumsum!(ptr, ptr)
    pairs = Matrix{Int32}(undef, 2, total)                                  # column t = (A entry, G entry): 8 bytes per product
    for (j, i) in enumerate(perm); pairs[1, j] = ai[i]; pairs[2, j] = gi[i]; end
    return (ROCVector(ptr), ROCMatrix(pairs), true)
end

# Values of the gathered rows, GPU to GPU (replaces execute_plan!(::MatrixPlan, B, target), src/sparse.jl:922-978, whose body
# copies every send range to the host (_copy_range_to_cpu), sends with host MPI and copies what arrives back -- on EVERY
# product).  The parent's MatrixPlan keeps describing the exchange: `send_ranges[i]` (ranges of B.nzval for rank_ids[i]),
# `recv_offsets[i]` / `length(recv_bufs[i])` (where recv_rank_ids[i]'s values land in the gathered array), `local_ranges`.
# Device form, built once per plan: the ranges expanded to one index list per neighbour feed the SpMV's own halo plan (width 1)
# over B.nzval; own ranges and the arrived segments are placed by two gather launches.  The twin of matmat.py
# MatrixPlan.gather_values, which the GPU tests hold to the oracle.  COLLECTIVE on first use (window attach).
const _rocm_matexec = IdDict{Any,Any}()   # reference MatrixPlan -> (halo handle, send_idx, local src, local dst, ghost src, ghost dst); freed by clear_rocm_plan_cache!
function _matrix_values!(gval::ROCVector{T}, plan::HPCLinearAlgebra.MatrixPlan, Bm::HPCSparseMatrix{T,Ti,B}) where {T<:Float64,Ti,B<:ROCBackend}
    st = get!(_rocm_matexec, plan) do
        comm = Bm.backend.comm
        send_lists = Vector{Int64}[reduce(vcat, (collect(Int64, rng) for rng in ranges); init=Int64[]) .- 1 for ranges in plan.send_ranges]   # 0-based positions in B.nzval
        recv_counts = Int64[length(buf) for buf in plan.recv_bufs]
        lsrc = Int64[]; ldst = Int64[]                                  # 1-based, as the plan holds them
        for (src_range, dst_off) in plan.local_ranges
            append!(lsrc, src_range); append!(ldst, dst_off:(dst_off + length(src_range) - 1))
        end
        gdst = Int64[]                                                  # ghost segment (neighbour order) -> gathered array
        for (off, cnt) in zip(plan.recv_offsets, recv_counts); append!(gdst, off:(off + cnt - 1)); end
        halo = Ref{Ptr{Cvoid}}(C_NULL)
        send_idx = ROCVector(reduce(vcat, send_lists; init=Int64[]))
        if !isempty(plan.rank_ids) || !isempty(plan.recv_rank_ids)
            AMDGPU.synchronize()
            # SINGLE-buffered (flags = 1): the plan is driven through halo_begin / halo_end and its ghost pointer is then a
            # constant, fetched once below -- on a double-buffered plan hpcla_halo_ghost_ptr reads the device step counter,
            # i.e. synchronises the device and copies 8 bytes to the host on EVERY call
            _check(@ccall(LIB.hpcla_halo_plan_create_ex(halo::Ptr{Ptr{Cvoid}}, _rccl(comm)::Ptr{Cvoid},
                   length(plan.rank_ids)::Cint, Int32.(plan.rank_ids)::Ptr{Int32},
                   Int64.(length.(send_lists))::Ptr{Int64}, _ptr(send_idx)::Ptr{Cvoid}, 1::Cint,
                   length(plan.recv_rank_ids)::Cint, Int32.(plan.recv_rank_ids)::Ptr{Int32},
                   recv_counts::Ptr{Int64}, 1::Cint, 1::Cint)::Cint), "hpcla_halo_plan_create_ex")
        end
        comm isa CommMPI && _attach_halo_window(_rccl(comm), halo[], comm.comm, comm_size(comm))
        ghost = Ref{Ptr{Cvoid}}(C_NULL); ng = Ref{Int64}(0)
        halo[] == C_NULL || _check(@ccall(LIB.hpcla_halo_ghost_ptr(halo[]::Ptr{Cvoid}, ghost::Ptr{Ptr{Cvoid}}, ng::Ptr{Int64})::Cint), "hpcla_halo_ghost_ptr")
        (halo[], send_idx, ROCVector(lsrc), ROCVector(ldst), ROCVector(collect(Int64, 1:length(gdst))), ROCVector(gdst), ghost[])
    end
    halo, _, lsrc, ldst, gsrc, gdst, ghost = st
    s = _stream()
    halo == C_NULL || _check(@ccall(LIB.hpcla_halo_begin(halo::Ptr{Cvoid}, _ptr(Bm.nzval)::Ptr{Cvoid}, s::Ptr{Cvoid})::Cint), "hpcla_halo_begin")
    # the own rows' values, under the exchange (1-based lists: index_base = 1)
    isempty(lsrc) || _check(@ccall(LIB.hpcla_gather_f64_i64(_ptr(Bm.nzval)::Ptr{Cvoid}, _ptr(lsrc)::Ptr{Cvoid}, _ptr(ldst)::Ptr{Cvoid},
                            _ptr(gval)::Ptr{Cvoid}, length(lsrc)::Int64, 1::Cint, s::Ptr{Cvoid})::Cint), "hpcla_gather_f64_i64")
    if halo != C_NULL
        _check(@ccall(LIB.hpcla_halo_end(halo::Ptr{Cvoid}, s::Ptr{Cvoid})::Cint), "hpcla_halo_end")
        isempty(gdst) || _check(@ccall(LIB.hpcla_gather_f64_i64(ghost::Ptr{Cvoid}, _ptr(gsrc)::Ptr{Cvoid}, _ptr(gdst)::Ptr{Cvoid},
                                _ptr(gval)::Ptr{Cvoid}, length(gdst)::Int64, 1::Cint, s::Ptr{Cvoid})::Cint), "hpcla_gather_f64_i64")
    end
    return gval
end

function Base.:*(A::HPCSparseMatrix{T,Ti,B}, Bm::HPCSparseMatrix{T,Ti,B}) where {T<:Float64,Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, Bm.backend)
    parent_path() = invoke(*, Tuple{HPCSparseMatrix{T,Ti,B},HPCSparseMatrix{T,Ti,B}} where {T,Ti,B}, A, Bm)   # PCIe: parent's host product (src/sparse.jl:991-1059) -- only for a row beyond the largest bin or another index type
    (Ti === Int32 || Ti === Int64) || return parent_path()
    plan = HPCLinearAlgebra.MatrixPlan(A, Bm)               # memoized, collective on first use (src/sparse.jl:900-910)
    st = get!(() -> _spgemm_symbolic(A, plan), _spgemm_cache, plan)
    st === nothing && return parent_path()                  # (decided collectively in _spgemm_symbolic)
    gval = ROCVector{T}(undef, max(length(plan.AT.nzval), 1))
    _matrix_values!(gval, plan, Bm)                         # values of the gathered rows, GPU to GPU (not the parent's host-staged execute_plan!)
    nrows = A.nrows_local
    if st.result === nothing
        # >>> plan time: the FIRST product on a structure builds C's structure (row pointers, column space) next to its values;
        # the struct's host fields (colptr, colval, col_indices: "always CPU" in the parent) come back once, here
        c_col_tmp = ROCVector{Int64}(undef, max(st.total_ub, 1)); c_val_tmp = ROCVector{T}(undef, max(st.total_ub, 1))
        _spgemm_numeric!(st, A, gval, st.ub_prefix, c_col_tmp, c_val_tmp)
        cnt_h = Array(st.cnt)[1:nrows]
        c_rowptr_h = vcat(Int64[0], cumsum(cnt_h)); nnzc = Int(c_rowptr_h[end])
        c_rowptr = ROCVector(c_rowptr_h)
        c_col = ROCVector{Int64}(undef, max(nnzc, 1)); c_val = ROCVector{T}(undef, nnzc)
        _check(@ccall(LIB.hpcla_spgemm_compact(_ptr(c_rowptr)::Ptr{Cvoid}, _ptr(st.ub_prefix)::Ptr{Cvoid}, nrows::Int64,
               _ptr(c_col_tmp)::Ptr{Cvoid}, _ptr(c_val_tmp)::Ptr{Cvoid}, _ptr(c_col)::Ptr{Cvoid}, _ptr(c_val)::Ptr{Cvoid},
               _stream()::Ptr{Cvoid})::Cint), "hpcla_spgemm_compact")
        # the result's column space (src/sparse.jl:1027-1040: unique(sort(rowval)) + a compress map) on the device
        c_col_h = Array(c_col)[1:nnzc]
        if nnzc == 0
            col_indices = Int[]; colval_target = ROCVector{Ti}(undef, 0); colval = Ti[]
        else
            lo, hi = extrema(c_col_h); window = Int64(hi - lo + 1)
            work = ROCVector{UInt8}(undef, @ccall LIB.hpcla_colspace_work_bytes(window::Int64)::Int64)
            ci_dev = ROCVector{Int64}(undef, window); colval_target = ROCVector{Ti}(undef, nnzc); ncomp = Ref{Int64}(0)
            if Ti === Int32
                _check(@ccall(LIB.hpcla_compress_columns_i32(_ptr(c_col)::Ptr{Cvoid}, nnzc::Int64, lo::Int64, window::Int64,
                       _ptr(colval_target)::Ptr{Cvoid}, 1::Cint, _ptr(ci_dev)::Ptr{Cvoid}, ncomp::Ptr{Int64}, _ptr(work)::Ptr{Cvoid},
                       _stream()::Ptr{Cvoid})::Cint), "hpcla_compress_columns_i32")
            else
                _check(@ccall(LIB.hpcla_compress_columns_i64(_ptr(c_col)::Ptr{Cvoid}, nnzc::Int64, lo::Int64, window::Int64,
                       _ptr(colval_target)::Ptr{Cvoid}, 1::Cint, _ptr(ci_dev)::Ptr{Cvoid}, ncomp::Ptr{Int64}, _ptr(work)::Ptr{Cvoid},
                       _stream()::Ptr{Cvoid})::Cint), "hpcla_compress_columns_i64")
            end
            col_indices = Int.(Array(ci_dev[1:ncomp[]])) .+ 1
            colval = Array(colval_target)
        end
        colptr = Ti.(c_rowptr_h .+ 1)
        c_row_h = [r for r in 1:nrows for _ in 1:cnt_h[r]]
        st.result = (c_rowptr64=c_rowptr, nnz=nnzc, col_indices=col_indices, colptr=colptr, colval=colval,
                     rowptr_target=HPCLinearAlgebra._to_target_device(colptr, A.backend.device), colval_target=colval_target,
                     scratch_col=c_col, c_col_h=c_col_h, c_row_h=c_row_h, hash=Ref{Any}(nothing))
        st.ub_prefix = nothing                              # upper-bound slots: first product only
        # <<< plan time
    else
        res = st.result
        c_val = ROCVector{T}(undef, res.nnz)
        st.repeats += 1
        if st.map === nothing && st.repeats >= 2            # a structure multiplied a third time will be multiplied again
            lists = get(ENV, "HPCLA_SPGEMM_MAP", "1") == "0" || res.nnz == 0 ? nothing :
                    _spgemm_product_lists(A, plan, res, Int(parse(Float64, get(ENV, "HPCLA_SPGEMM_MAP_MAX", "5e7"))))
            st.map = lists === nothing ? :none : lists
        end
        if st.map isa Tuple
            _spgemm_touch_lists!(st)
            ptr, pairs, ptr64 = st.map
            _check(@ccall(LIB.hpcla_spgemm_numeric_mapped_f64(_ptr(ptr)::Ptr{Cvoid}, (ptr64 ? 1 : 0)::Cint, _ptr(pairs)::Ptr{Cvoid},
                   _ptr(A.nzval)::Ptr{Cvoid}, _ptr(gval)::Ptr{Cvoid}, _ptr(c_val)::Ptr{Cvoid}, res.nnz::Int64,
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_spgemm_numeric_mapped_f64")
        else
            # the rows' final offsets are known: the numeric kernels write the compacted arrays directly
            _spgemm_numeric!(st, A, gval, res.c_rowptr64, res.scratch_col, c_val)
        end
    end
    res = st.result
    C = HPCSparseMatrix{T,Ti,B}(res.hash[], A.row_partition, Bm.col_partition, res.col_indices, res.colptr, res.colval, c_val,
                                nrows, length(res.col_indices), nothing, nothing, res.rowptr_target, res.colval_target, A.backend)
    res.hash[] === nothing && (res.hash[] = HPCLinearAlgebra._ensure_hash(C))   # collective, once per structure (device digest)
    return C
end

# ==== Float32 backends (csrc/f32.hip) ====================================================================================
# The parent is generic in T and its GPU test configurations run Float32 as well as Float64 (test/test_utils.jl:62-80).
# The methods above are Float64's; these give a Float32 backend the same path instead of the parent's host-staged one:
# A*x, mul!, A*B with a dense B, dot, norm (p = 1, 2, Inf), sum, maximum, minimum.  Row sums run in Float32 in stored order
# (the bits of _spmv_kernel!, src/sparse.jl:2055-2066, with T = Float32); reductions are formed and all-reduced in double
# and rounded to Float32 once.  Ghost values travel widened to Float64 (exact both ways), so every halo transport is the
# Float64 one.  Everything else (CG pieces, transposes, sparse products and sums, repartition) keeps the parent's generic
# methods for Float32.
const _stage32 = IdDict{Any,Any}()      # device plan -> staging vector (ROCVector{Float64}) of its Float32 / column-major exchanges
_stage(d, n::Int) = (st = get(_stage32, d, nothing); (st === nothing || length(st) < n) ? (_stage32[d] = AMDGPU.zeros(Float64, max(n, 1))) : st)

# y (nrows_local values at `yp`) = A * (x: n_own values at `xp`): hpcla_spmv_dist_f32_* -- the exchange (values widened into
# the plan's staging vector), the interior blocks overlapping it, the boundary blocks behind it, in one call
function _spmv_f32!(yp::Ptr{Cvoid}, A::HPCSparseMatrix{Float32,Ti,B}, xp::Ptr{Cvoid}, d::ROCVectorPlan{Tk}) where {Ti,Tk,B<:ROCBackend}
    nnz = length(A.nzval)
    stage = d.halo == C_NULL ? C_NULL : _ptr(_stage(d, d.n_own))
    if Tk === Int32
        _check(@ccall(LIB.hpcla_spmv_dist_f32_i32(d.halo::Ptr{Cvoid}, _ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, xp::Ptr{Cvoid}, d.n_own::Int64, yp::Ptr{Cvoid}, A.nrows_local::Int64, nnz::Int64, 0::Cint,
               _ptr(d.interior)::Ptr{Cvoid}, length(d.interior)::Int64, _ptr(d.boundary)::Ptr{Cvoid}, length(d.boundary)::Int64,
               stage::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmv_dist_f32_i32")
    else
        _check(@ccall(LIB.hpcla_spmv_dist_f32_i64(d.halo::Ptr{Cvoid}, _ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, xp::Ptr{Cvoid}, d.n_own::Int64, yp::Ptr{Cvoid}, A.nrows_local::Int64, nnz::Int64, 0::Cint,
               _ptr(d.interior)::Ptr{Cvoid}, length(d.interior)::Int64, _ptr(d.boundary)::Ptr{Cvoid}, length(d.boundary)::Int64,
               stage::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmv_dist_f32_i64")
    end
    return
end

function _spmv_dist!(y::ROCVector{Float32}, A::HPCSparseMatrix{Float32,Ti,B}, x::HPCVector{Float32,B}) where {Ti,B<:ROCBackend}
    plan = get_vector_plan(A, x)
    _spmv_f32!(_ptr(y), A, _ptr(x.v), _device_plan(A, x, plan))
    return plan
end

function Base.:*(A::HPCSparseMatrix{Float32,Ti,B}, x::HPCVector{Float32,B}) where {Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, x.backend)
    y_local = similar(A.nzval, A.nrows_local)
    plan = _spmv_dist!(y_local, A, x)
    if plan.result_partition_hash === nothing
        plan.result_partition_hash = compute_partition_hash(A.row_partition)
        plan.result_partition = copy(A.row_partition)
    end
    return HPCVector{Float32,B}(plan.result_partition_hash, plan.result_partition, y_local, A.backend)
end

function LinearAlgebra.mul!(y::HPCVector{Float32,B}, A::HPCSparseMatrix{Float32,Ti,B}, x::HPCVector{Float32,B}) where {Ti,B<:ROCBackend}
    _spmv_dist!(y.v, A, x)
    return y
end

# A * B, B::HPCMatrix (src/sparse.jl:2391-2413): like the Float64 product -- banded structure: on the column-major blocks as
# they are (_spmm_colmajor); unstructured: B converted once to row-major rows (hpcla_transpose_f32), whose ghost rows travel
# widened in ONE width-k exchange that the interior blocks overlap, the row-major Float32 kernels, C converted back.
function _spmm_split_f32!(Crow, A::HPCSparseMatrix{Float32,Ti,B}, rp0, colval_split, n_own::Int, Brow, ghost::Ptr{Cvoid}, k::Int, blocks) where {Ti,B}
    blocks !== nothing && isempty(blocks) && return
    nnz = length(A.nzval); nb = _len(blocks)
    if eltype(rp0) === Int32
        _check(@ccall(LIB.hpcla_spmm_split_f32_i32(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, k::Int64, ghost::Ptr{Cvoid}, k::Int64, n_own::Int64,
               _ptr(Crow)::Ptr{Cvoid}, k::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint,
               _ptr(blocks)::Ptr{Cvoid}, nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_f32_i32")
    else
        _check(@ccall(LIB.hpcla_spmm_split_f32_i64(_ptr(rp0)::Ptr{Cvoid}, _ptr(colval_split)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, k::Int64, ghost::Ptr{Cvoid}, k::Int64, n_own::Int64,
               _ptr(Crow)::Ptr{Cvoid}, k::Int64, A.nrows_local::Int64, nnz::Int64, k::Cint, 0::Cint,
               _ptr(blocks)::Ptr{Cvoid}, nb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_split_f32_i64")
    end
end

function Base.:*(A::HPCSparseMatrix{Float32,Ti,B}, M::HPCMatrix{Float32,B}) where {Ti,B<:ROCBackend}
    assert_backends_compatible(A.backend, M.backend)
    nloc, k = size(M.A)
    plan, d = _spmm_vector_plan(A, M)
    _banded(A, d) && return _spmm_colmajor(A, M, plan, d)
    Brow = ROCMatrix{Float32}(undef, k, nloc)             # k x nloc column-major == nloc x k row-major
    _check(@ccall(LIB.hpcla_transpose_f32(_ptr(M.A)::Ptr{Cvoid}, max(nloc, 1)::Int64, 1::Cint, _ptr(Brow)::Ptr{Cvoid}, k::Int64,
           0::Cint, nloc::Int64, k::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_transpose_f32")
    Crow = ROCMatrix{Float32}(undef, k, A.nrows_local)
    if comm_size(A.backend.comm) == 1
        _spmm_split_f32!(Crow, A, d.rowptr0, d.colval_split, d.n_own, Brow, C_NULL, k, nothing)
    else
        # (every rank, with or without neighbours: the entry's first use is collective)
        halo, interior, boundary, _, ghost, colval_split, rp0 =
            _spmm_halo(A, plan, d, M.row_partition, k, (@ccall LIB.hpcla_spmv_rows_per_block()::Cint))
        if halo == C_NULL
            _spmm_split_f32!(Crow, A, rp0, colval_split, d.n_own, Brow, C_NULL, k, nothing)
        else
            _check(@ccall(LIB.hpcla_halo_begin_f32(halo::Ptr{Cvoid}, _ptr(Brow)::Ptr{Cvoid}, _ptr(_stage(d, d.n_own * k))::Ptr{Cvoid},
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_begin_f32")
            _spmm_split_f32!(Crow, A, rp0, colval_split, d.n_own, Brow, C_NULL, k, interior)   # overlaps the exchange
            _check(@ccall(LIB.hpcla_halo_end(halo::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_halo_end")
            _spmm_split_f32!(Crow, A, rp0, colval_split, d.n_own, Brow, ghost, k, boundary)
        end
    end
    C = ROCMatrix{Float32}(undef, A.nrows_local, k)
    _check(@ccall(LIB.hpcla_transpose_f32(_ptr(Crow)::Ptr{Cvoid}, k::Int64, 0::Cint, _ptr(C)::Ptr{Cvoid},
           max(A.nrows_local, 1)::Int64, 1::Cint, A.nrows_local::Int64, k::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_transpose_f32")
    return _spmm_result(A, C, k)
end

function _reduce_f32(sym::Symbol, x::HPCVector{Float32}, y=nothing, negate::Int=0)
    work, out = _scratch(); c = _rccl(x.backend.comm); n = length(x.v)
    if sym === :dot
        _check(@ccall(LIB.hpcla_dot_f32(c::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, _ptr(y.v)::Ptr{Cvoid}, n::Int64,
               _ptr(out)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_dot_f32")
    elseif sym === :nrm2sq
        _check(@ccall(LIB.hpcla_nrm2sq_f32(c::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_nrm2sq_f32")
    elseif sym === :asum
        _check(@ccall(LIB.hpcla_asum_f32(c::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_asum_f32")
    elseif sym === :amax
        _check(@ccall(LIB.hpcla_amax_f32(c::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_amax_f32")
    elseif sym === :sum
        _check(@ccall(LIB.hpcla_sum_f32(c::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, n::Int64, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_sum_f32")
    else
        _check(@ccall(LIB.hpcla_maxval_f32(c::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, n::Int64, negate::Cint, _ptr(out)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_maxval_f32")
    end
    return _host_scalar(out, x.backend)              # a double; the callers round to Float32 once
end
function LinearAlgebra.dot(x::HPCVector{Float32,B}, y::HPCVector{Float32,B}) where {B<:ROCBackend}
    assert_backends_compatible(x.backend, y.backend)
    x.structural_hash == y.structural_hash || (y = HPCLinearAlgebra.repartition(y, x.partition))   # PCIe: all of y, both ways, ONLY when the partitions differ -- the parent's host-staged repartition (no Float32 device exchange in this file)
    return Float32(_reduce_f32(:dot, x, y))
end
function LinearAlgebra.norm(v::HPCVector{Float32,B}, p::Real=2) where {B<:ROCBackend}
    p == 2 && return Float32(sqrt(_reduce_f32(:nrm2sq, v)))
    p == 1 && return Float32(_reduce_f32(:asum, v))
    p == Inf && return Float32(_reduce_f32(:amax, v))
    return invoke(LinearAlgebra.norm, Tuple{HPCVector,Real}, v, p)        # PCIe: parent's generic method (p other than 1, 2, Inf) -- whatever the array package's norm moves
end
Base.sum(v::HPCVector{Float32,B}) where {B<:ROCBackend} = Float32(_reduce_f32(:sum, v))
Base.maximum(v::HPCVector{Float32,B}) where {B<:ROCBackend} = Float32(_reduce_f32(:max, v, nothing, 0))
Base.minimum(v::HPCVector{Float32,B}) where {B<:ROCBackend} = Float32(-_reduce_f32(:max, v, nothing, 1))

# ---- execute_plan!(::VectorPlan, x) on the device  (replaces src/vectors.jl:394-463 for every OTHER caller of
# the plan: vector operands with different partitions :870-876, dense A*x, ...; A*x above never needs `gathered`)
# gathered[local_dst] = x[local_src] and gathered[recv_perm[i]] = what neighbour i sent, GPU to GPU; the CPU
# staging buffer `gathered_cpu` is never touched.  Collective like the reference's.
const _rocm_exec = IdDict{Any,Any}()      # reference plan -> (halo handle, device index lists, send_idx, ghost pointer); freed by clear_rocm_plan_cache!
function HPCLinearAlgebra.execute_plan!(plan::HPCLinearAlgebra.VectorPlan{T,Ti,<:ROCVector},
                                        x::HPCVector{T,B}) where {T<:Float64,Ti,B<:ROCBackend}
    st = get!(_rocm_exec, plan) do
        halo = Ref{Ptr{Cvoid}}(C_NULL)
        send_idx = ROCVector(Int64.(reduce(vcat, plan.send_indices; init=Ti[])) .- 1)      # 0-based, kept alive with the plan
        if !isempty(plan.send_rank_ids) || !isempty(plan.recv_rank_ids)
            AMDGPU.synchronize()
            # SINGLE-buffered (flags = 1): begin / end driven; the ghost pointer is a constant fetched once below (a
            # double-buffered plan's hpcla_halo_ghost_ptr synchronises the device and reads 8 bytes back on every call)
            _check(@ccall(LIB.hpcla_halo_plan_create_ex(halo::Ptr{Ptr{Cvoid}}, _rccl(x.backend.comm)::Ptr{Cvoid},
                   length(plan.send_rank_ids)::Cint, Int32.(plan.send_rank_ids)::Ptr{Int32},
                   Int64.(length.(plan.send_indices))::Ptr{Int64}, _ptr(send_idx)::Ptr{Cvoid}, 1::Cint,
                   length(plan.recv_rank_ids)::Cint, Int32.(plan.recv_rank_ids)::Ptr{Int32},
                   Int64.(length.(plan.recv_perm))::Ptr{Int64}, 1::Cint, 1::Cint)::Cint), "hpcla_halo_plan_create_ex")
        end
        x.backend.comm isa CommMPI &&
            _attach_halo_window(_rccl(x.backend.comm), halo[], x.backend.comm.comm, comm_size(x.backend.comm))
        perm = Int64.(reduce(vcat, plan.recv_perm; init=Ti[]))
        ghost = Ref{Ptr{Cvoid}}(C_NULL); ng = Ref{Int64}(0)
        halo[] == C_NULL || _check(@ccall(LIB.hpcla_halo_ghost_ptr(halo[]::Ptr{Cvoid}, ghost::Ptr{Ptr{Cvoid}}, ng::Ptr{Int64})::Cint),
                                   "hpcla_halo_ghost_ptr")
        (halo[], ROCVector(Int64.(plan.local_src_indices)), ROCVector(Int64.(plan.local_dst_indices)),
         ROCVector(perm), ROCVector(collect(Int64, 1:length(perm))), send_idx, ghost[])
    end
    halo, src, dst, perm, ident, _, ghost = st
    s = _stream()
    # (a plan of this file's VectorPlan constructor starts without its `gathered` buffer: A * x never reads it)
    n_gathered = length(plan.local_dst_indices) + sum(length, plan.recv_perm; init=0)
    length(plan.gathered) == n_gathered || (plan.gathered = similar(x.v, n_gathered))
    halo == C_NULL || _check(@ccall(LIB.hpcla_halo_begin(halo::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid}, s::Ptr{Cvoid})::Cint),
                             "hpcla_halo_begin")
    # the own part, under the exchange: 1-based lists as they stand (index_base = 1)
    isempty(src) || _check(@ccall(LIB.hpcla_gather_f64_i64(_ptr(x.v)::Ptr{Cvoid}, _ptr(src)::Ptr{Cvoid}, _ptr(dst)::Ptr{Cvoid},
                           _ptr(plan.gathered)::Ptr{Cvoid}, length(src)::Int64, 1::Cint, s::Ptr{Cvoid})::Cint),
                           "hpcla_gather_f64_i64")
    if halo != C_NULL
        _check(@ccall(LIB.hpcla_halo_end(halo::Ptr{Cvoid}, s::Ptr{Cvoid})::Cint), "hpcla_halo_end")
        isempty(perm) || _check(@ccall(LIB.hpcla_gather_f64_i64(ghost::Ptr{Cvoid}, _ptr(ident)::Ptr{Cvoid},
                                _ptr(perm)::Ptr{Cvoid}, _ptr(plan.gathered)::Ptr{Cvoid}, length(perm)::Int64, 1::Cint,
                                s::Ptr{Cvoid})::Cint), "hpcla_gather_f64_i64")
    end
    return plan.gathered
end

# ---- freeing the device halves of the plans ------------------------------------------------------------------
# Explicit and collective, never from a finalizer (the handles own device memory, IPC mappings and a stream; the
# CUDA extension states the same rule for its communicators, ext/HPCLinearAlgebraCUDAExt.jl:9-10, 384-386).
# Call it wherever clear_plan_cache!() is called (src/HPCLinearAlgebra.jl:181-201 empties the reference plans
# these entries are keyed on); INTEGRATION.md shows the one-line hook for the parent.
function clear_rocm_plan_cache!()
    destroy(h) = h == C_NULL || @ccall LIB.hpcla_halo_plan_destroy(h::Ptr{Cvoid})::Cint
    AMDGPU.synchronize()
    for d in values(_rocm_plans); d isa ROCVectorPlan && destroy(d.halo); end
    for st in values(_spmm_plans); destroy(st[1]); end
    for st in values(_rocm_exec); destroy(st[1]); end
    for st in values(_rocm_matexec); destroy(st[1]); end
    for d in values(_rocm_plans)    # the plans' rowptr copies carry the block-order hints: removed before the arrays go
        d isa ROCVectorPlan && @ccall LIB.hpcla_spmv_block_order_hint(_ptr(d.rowptr0)::Ptr{Cvoid}, 0::Cint)::Cint
    end
    for rp0 in keys(_spmm_order_in_force); @ccall LIB.hpcla_spmm_block_order_hint(_ptr(rp0)::Ptr{Cvoid}, 0::Cint)::Cint; end
    empty!(_rocm_plans); empty!(_spmm_plans); empty!(_rocm_exec); empty!(_rocm_matexec); empty!(_merge_lists); empty!(_spmm_runs_cache); empty!(_stage32); empty!(_banded_cache); empty!(_spmm_cm_tuned); empty!(_spmm_order_in_force)
    empty!(_spgemm_cache); empty!(_spgemm_map_lru); empty!(_spmm_t_plans)
    return nothing
end

# ---- repartition(x, p)  (replaces the CPU-staged execute_plan! of src/vectors.jl:624-671) ---------------
# The plan is the reference's own VectorRepartitionPlan; its range lists go to the C ABI unchanged
# (1-based -> 0-based offsets).  Data moves GPU to GPU, no _ensure_cpu / _values_to_backend round trip.
function HPCLinearAlgebra.execute_plan!(plan::HPCLinearAlgebra.VectorRepartitionPlan{T},
                                        x::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend}
    out = AMDGPU.zeros(T, plan.result_local_size)
    send_ranks = Cint.(plan.send_rank_ids)
    send_off = Int64[first(r) - 1 for r in plan.send_ranges]
    send_cnt = Int64[length(r) for r in plan.send_ranges]
    recv_ranks = Cint.(plan.recv_rank_ids)
    recv_off = Int64[o - 1 for o in plan.recv_offsets]
    recv_cnt = Int64.(plan.recv_counts)
    lsrc = isempty(plan.local_src_range) ? 0 : first(plan.local_src_range) - 1
    ldst = isempty(plan.local_src_range) ? 0 : plan.local_dst_offset - 1
    _check(@ccall(LIB.hpcla_exchange_ranges_f64(_rccl(x.backend.comm)::Ptr{Cvoid}, _ptr(x.v)::Ptr{Cvoid},
           _ptr(out)::Ptr{Cvoid}, length(send_ranks)::Cint, send_ranks::Ptr{Cint}, send_off::Ptr{Int64},
           send_cnt::Ptr{Int64}, length(recv_ranks)::Cint, recv_ranks::Ptr{Cint}, recv_off::Ptr{Int64},
           recv_cnt::Ptr{Int64}, lsrc::Int64, ldst::Int64, length(plan.local_src_range)::Int64, 1::Cint,
           _stream()::Ptr{Cvoid})::Cint), "hpcla_exchange_ranges_f64")
    return HPCVector{T,B}(plan.result_partition_hash, plan.result_partition, out, x.backend)
end

# ---- A + B / A - B value pass  (replaces execute_addition!/execute_subtraction!, src/sparse.jl:1311-1375) --
# One coalesced pass over the merged pattern instead of three index-mapped kernels: per result entry its
# 0-based position in A.nzval / B.nzval, or -1.  Built once per AdditionPlan from the plan's own groups.
const _merge_lists = IdDict{Any,Any}()
function _merge_lists_for(plan::HPCLinearAlgebra.AdditionPlan{T,Ti}) where {T,Ti}
    get!(_merge_lists, plan) do
        n = Int(plan.colptr[end]) - 1
        ia = fill(Int32(-1), n); ib = fill(Int32(-1), n)
        ia[Array(plan.A_only_dst)] .= Int32.(Array(plan.A_only_src) .- 1)
        ib[Array(plan.B_only_dst)] .= Int32.(Array(plan.B_only_src) .- 1)
        ia[Array(plan.both_dst)] .= Int32.(Array(plan.both_A_src) .- 1)
        ib[Array(plan.both_dst)] .= Int32.(Array(plan.both_B_src) .- 1)
        (ROCArray(ia), ROCArray(ib))
    end
end
function _merge_combine!(nzval::ROCVector{Float64}, plan, A_nzval::ROCVector{Float64}, B_nzval::ROCVector{Float64}, sub::Bool)
    ia, ib = _merge_lists_for(plan)
    _check(@ccall(LIB.hpcla_merge_combine_f64_i32(_ptr(nzval)::Ptr{Cvoid}, _ptr(A_nzval)::Ptr{Cvoid}, _ptr(ia)::Ptr{Cvoid},
           _ptr(B_nzval)::Ptr{Cvoid}, _ptr(ib)::Ptr{Cvoid}, length(nzval)::Int64, (sub ? 1 : 0)::Cint,
           _stream()::Ptr{Cvoid})::Cint), "hpcla_merge_combine_f64_i32")
    return nzval
end
HPCLinearAlgebra.execute_addition!(nzval::ROCVector{Float64}, plan::HPCLinearAlgebra.AdditionPlan,
                                   A_nzval::ROCVector{Float64}, B_nzval::ROCVector{Float64}) =
    _merge_combine!(nzval, plan, A_nzval, B_nzval, false)
HPCLinearAlgebra.execute_subtraction!(nzval::ROCVector{Float64}, plan::HPCLinearAlgebra.AdditionPlan,
                                      A_nzval::ROCVector{Float64}, B_nzval::ROCVector{Float64}) =
    _merge_combine!(nzval, plan, A_nzval, B_nzval, true)

# ---- dense A * x and transpose(A) * x  (replace src/dense.jl:614-658, 1210-1261) ----------------------------
# HPCMatrix stores its block column-major (Julia Matrix): a column-major (nloc x n) block IS the row-major
# (n x nloc) block of its transpose, so the two entry points swap roles -- A*x reads A.A through the
# column-sum kernel and transpose(A)*x through the row-dot kernel; no relayout.
function Base.:*(A::HPCMatrix{T,B}, x::HPCVector{T,B}) where {T<:Float64,B<:ROCBackend}
    # several ranks: the parent's method (src/dense.jl:614-658) gathers x through execute_plan!(::VectorPlan, x) --
    # the device exchange above -- and multiplies the local block with the array package's gemv
    comm_size(A.backend.comm) == 1 || return invoke(Base.:*, Tuple{HPCMatrix,HPCVector}, A, x)   # PCIe: parent's method at N > 1 -- no host copy in its body: x arrives through this file's device execute_plan!
    nloc, n = size(A.A)
    y = AMDGPU.zeros(T, nloc)
    work = AMDGPU.zeros(UInt8, @ccall LIB.hpcla_gemv_t_work_bytes(n::Int64, nloc::Int64)::Int64)
    # y[i] = sum_j A.A[i,j] x[j]: column sums of the row-major (n x nloc) view weighted by x
    _check(@ccall(LIB.hpcla_gemv_t_rowmajor_f64(_ptr(A.A)::Ptr{Cvoid}, nloc::Int64, n::Int64, nloc::Int64,
           _ptr(x.v)::Ptr{Cvoid}, _ptr(y)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint),
           "hpcla_gemv_t_rowmajor_f64")
    return HPCVector{T,B}(compute_partition_hash(A.row_partition), A.row_partition, y, A.backend)
end

# ---- transpose(X) * Y for dense blocks  (replaces src/dense.jl:1286-1310) --------------------------------------------
# The parent builds the m x k product one column at a time: k products transpose(X) * Y[:, j], each a column copy, a read of
# all of X and a host all-reduce.  Here ONE hpcla_gram_* call reads the two column-major blocks as they are
# (HPCLA_LAYOUT_COL, leading dimension = the local row count) and all-reduces the m x k doubles on the device; X === Y reads
# the block once and gives an exactly symmetric C.  This rank's rows of C (X.col_partition) are copied column-major on the
# device by hpcla_transpose_f64 (Float32: rounded once, after the all-reduce), and the result is built with the inner
# constructor as the parent's HPCMatrix_local would describe it (rows = X.col_partition, columns = uniform_partition(k)).
function _gram(X::HPCMatrix{T,B}, M::HPCMatrix{T,B}) where {T,B<:ROCBackend}
    assert_backends_compatible(X.backend, M.backend)
    X.row_partition[end] == M.row_partition[end] ||
        error("dimension mismatch: transpose(X) has $(X.row_partition[end]) columns, Y has $(M.row_partition[end]) rows")
    same = X === M
    X.row_partition == M.row_partition || (M = HPCLinearAlgebra.repartition(M, X.row_partition))   # PCIe: all of Y, both ways, ONLY when the row partitions differ -- the parent's host-staged repartition
    nloc, m = size(X.A)
    k = size(M.A, 2)
    nranks, rank = comm_size(X.backend.comm), comm_rank(X.backend.comm)
    C = AMDGPU.zeros(Float64, m * k)                  # row-major m x k
    work = AMDGPU.zeros(UInt8, @ccall LIB.hpcla_gram_work_bytes(nloc::Int64, m::Int64, k::Int64)::Int64)
    Y = same ? X : M
    ldx, ldy = max(nloc, 1), max(size(Y.A, 1), 1)
    # no rows to read: one non-NULL pointer for both says X'X (C is then mirrored like on the other ranks), NULL otherwise
    xp, yp = nloc == 0 ? (same ? (_ptr(C), _ptr(C)) : (C_NULL, C_NULL)) : (_ptr(X.A), _ptr(Y.A))
    if T === Float32
        _check(@ccall(LIB.hpcla_gram_f32(_rccl(X.backend.comm)::Ptr{Cvoid}, xp::Ptr{Cvoid}, ldx::Int64, 1::Cint,
               yp::Ptr{Cvoid}, ldy::Int64, 1::Cint, nloc::Int64, m::Int64, k::Int64, _ptr(C)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_gram_f32")
    else
        _check(@ccall(LIB.hpcla_gram_f64(_rccl(X.backend.comm)::Ptr{Cvoid}, xp::Ptr{Cvoid}, ldx::Int64, 1::Cint,
               yp::Ptr{Cvoid}, ldy::Int64, 1::Cint, nloc::Int64, m::Int64, k::Int64, _ptr(C)::Ptr{Cvoid},
               _ptr(work)::Ptr{Cvoid}, _stream()::Ptr{Cvoid})::Cint), "hpcla_gram_f64")
    end
    lo, hi = X.col_partition[rank + 1], X.col_partition[rank + 2]
    own = AMDGPU.zeros(Float64, hi - lo, k)
    if hi > lo                                        # own rows lo:hi-1 of the row-major C -> column-major
        _check(@ccall(LIB.hpcla_transpose_f64((_ptr(C) + 8 * (lo - 1) * k)::Ptr{Cvoid}, k::Int64, 0::Cint, _ptr(own)::Ptr{Cvoid},
               (hi - lo)::Int64, 1::Cint, (hi - lo)::Int64, k::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_transpose_f64")
    end
    local_C = T === Float64 ? own : T.(own)           # Float32 rounds here, once
    return HPCMatrix{T,B}(nothing, copy(X.col_partition), HPCLinearAlgebra.uniform_partition(k, nranks), local_C, X.backend)
end
function Base.:*(At::Transpose{Float64,HPCMatrix{Float64,B}}, M::HPCMatrix{Float64,B}) where {B<:ROCBackend}
    return _gram(LinearAlgebra.transpose(At), M)          # the transpose of a lazy transpose is its parent
end
function Base.:*(At::Transpose{Float32,HPCMatrix{Float32,B}}, M::HPCMatrix{Float32,B}) where {B<:ROCBackend}
    return _gram(LinearAlgebra.transpose(At), M)          # the transpose of a lazy transpose is its parent
end

# ---- X * A and transpose(X) * A for a sparse A  (replaces src/sparse.jl:3617-3690) -------------------------------------------
# The parent loops over the n columns of A: per column a sparse column extraction across ranks, a dense mat-vec with its own
# all-reduce and a copy of the column to the host -- n distributed operations.  Here ONE transposed SpMM (hpcla_spmm_t_f64_*)
# forms W = A^T X from this rank's rows of A over the split column space of the SpMV plan for x on A.col_partition; with
# N > 1 the ghost rows of W are partial sums of other ranks' columns: they go back to their owners
# (hpcla_exchange_ranges_f64, the plan's lists run backwards) and hpcla_spmm_t_accumulate_f64 adds them in ascending rank
# order.  The result's rows are then collected with one more range exchange.  Float64 only (Float32 keeps the parent's
# method).
const _spmm_t_plans = IdDict{Any,Any}()    # reference plan -> device CSC + reverse lists; freed by clear_rocm_plan_cache!

function _spmm_t_plan(A::HPCSparseMatrix{T,Ti,B}) where {T,Ti,B<:ROCBackend}
    probe = HPCVector{T,B}(_partition_hash(A.col_partition), A.col_partition, similar(A.nzval, 0), A.backend)   # plan key only
    plan = get_vector_plan(A, probe)
    get!(_spmm_t_plans, plan) do
        rank = comm_rank(A.backend.comm)
        n_own = A.col_partition[rank + 2] - A.col_partition[rank + 1]
        # the device half is shared with A * x on this structure: hand it n_own readable values, so that its block-order
        # measurement runs whichever product builds it first (the values are multiplied and discarded)
        xz = AMDGPU.zeros(T, max(n_own, 1))
        d = Base.GC.@preserve xz _device_plan(A, A.col_partition, n_own, n_own > 0 ? _ptr(xz) : C_NULL, plan)
        Tk = eltype(d.colval_split)
        nnz = length(A.nzval)
        seg = Int64.(length.(plan.recv_perm))
        n_split = n_own + sum(seg; init=0)
        colptr = ROCVector{Tk}(undef, n_split + 1)
        rowidx = ROCVector{Tk}(undef, max(nnz, 1))
        perm = ROCVector{Tk}(undef, max(nnz, 1))
        wb = @ccall LIB.hpcla_spmm_t_struct_work_bytes(nnz::Int64, n_split::Int64, (Tk === Int64 ? 1 : 0)::Cint)::Int64
        wb >= 0 || error("hpcla_spmm_t_struct_work_bytes: bad size")
        work = AMDGPU.zeros(UInt8, max(wb, 1))
        if Tk === Int64
            _check(@ccall(LIB.hpcla_spmm_t_struct_i64(_ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
                   A.nrows_local::Int64, nnz::Int64, n_split::Int64, _ptr(colptr)::Ptr{Cvoid}, _ptr(rowidx)::Ptr{Cvoid},
                   _ptr(perm)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid}, wb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_t_struct_i64")
        else
            _check(@ccall(LIB.hpcla_spmm_t_struct_i32(_ptr(d.rowptr0)::Ptr{Cvoid}, _ptr(d.colval_split)::Ptr{Cvoid},
                   A.nrows_local::Int64, nnz::Int64, n_split::Int64, _ptr(colptr)::Ptr{Cvoid}, _ptr(rowidx)::Ptr{Cvoid},
                   _ptr(perm)::Ptr{Cvoid}, _ptr(work)::Ptr{Cvoid}, wb::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_t_struct_i32")
        end
        # reverse halo: ghost segment i (rows of W) back to recv_rank_ids[i]; received in the forward send_indices order
        back_off = Int64.(n_own .+ cumsum([0; seg])[1:end-1])
        from_cnt = Int64.(length.(plan.send_indices))
        from_off = Int64.(cumsum([0; from_cnt])[1:end-1])
        rows = Int64.(reduce(vcat, plan.send_indices; init=Ti[]) .- 1)          # 0-based own rows, ascending sender rank
        order = sortperm(rows; alg=MergeSort)                                    # stable: peers stay in ascending rank
        urows = unique(rows[order])
        ptr = Int64[searchsortedfirst(rows[order], r) - 1 for r in urows]
        acc = isempty(urows) ? nothing :
              (ROCVector(urows), ROCVector([ptr; length(rows)]), ROCVector(Int64.(order .- 1)), length(urows))
        AMDGPU.synchronize()
        (colptr=colptr, rowidx=rowidx, perm=perm, Tk=Tk, n_own=n_own, n_split=n_split,
         back_ranks=Cint.(plan.recv_rank_ids), back_off=back_off, back_cnt=seg,
         from_ranks=Cint.(plan.send_rank_ids), from_off=from_off, from_cnt=from_cnt, n_recv=sum(from_cnt; init=0), acc=acc)
    end
end

# W = A^T X: X this rank's rows (A.nrows_local x m) read as ROWS (row-major, leading dimension ldx); W row-major (ldw = m)
function _spmm_t_product!(W::ROCArray{Float64}, A::HPCSparseMatrix{T,Ti,B}, st, xp::Ptr{Cvoid}, ldx::Int, m::Int) where {T,Ti,B}
    if st.Tk === Int64
        _check(@ccall(LIB.hpcla_spmm_t_f64_i64(_ptr(st.colptr)::Ptr{Cvoid}, _ptr(st.rowidx)::Ptr{Cvoid}, _ptr(st.perm)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, st.n_split::Int64, xp::Ptr{Cvoid}, ldx::Int64, 0::Cint, m::Int64,
               _ptr(W)::Ptr{Cvoid}, max(m, 1)::Int64, 0::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_t_f64_i64")
    else
        _check(@ccall(LIB.hpcla_spmm_t_f64_i32(_ptr(st.colptr)::Ptr{Cvoid}, _ptr(st.rowidx)::Ptr{Cvoid}, _ptr(st.perm)::Ptr{Cvoid},
               _ptr(A.nzval)::Ptr{Cvoid}, st.n_split::Int64, xp::Ptr{Cvoid}, ldx::Int64, 0::Cint, m::Int64,
               _ptr(W)::Ptr{Cvoid}, max(m, 1)::Int64, 0::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_t_f64_i32")
    end
    return W
end

# one range exchange of doubles on the task's stream (0-based offsets and counts, in units of `width` doubles)
function _ranges!(comm, src, dst, sr, so, sc, rr, ro, rc, lsrc, ldst, lcnt, width)
    _check(@ccall(LIB.hpcla_exchange_ranges_f64(_rccl(comm)::Ptr{Cvoid}, _ptr(src)::Ptr{Cvoid}, _ptr(dst)::Ptr{Cvoid},
           length(sr)::Cint, Cint.(sr)::Ptr{Cint}, Int64.(so)::Ptr{Int64}, Int64.(sc)::Ptr{Int64}, length(rr)::Cint,
           Cint.(rr)::Ptr{Cint}, Int64.(ro)::Ptr{Int64}, Int64.(rc)::Ptr{Int64}, Int64(lsrc)::Int64, Int64(ldst)::Int64,
           Int64(lcnt)::Int64, Cint(width)::Cint, _stream()::Ptr{Cvoid})::Cint), "hpcla_exchange_ranges_f64")
end

# strided block copy on the device: rows x cols, row-major source (ld ls) -> row-major destination (ld ld)
_place!(src::Ptr{Cvoid}, ls, dst::Ptr{Cvoid}, ld, rows, cols) = rows > 0 && cols > 0 &&
    _check(@ccall(LIB.hpcla_transpose_f64(src::Ptr{Cvoid}, Int64(ls)::Int64, 0::Cint, dst::Ptr{Cvoid}, Int64(ld)::Int64, 0::Cint,
           Int64(rows)::Int64, Int64(cols)::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_transpose_f64")

# transpose(X) * A for X's rows as ROWS (xp, ldx; aligned with A's rows) -> this rank's rows Q of the m x n product, column-major
function _spmm_t_result(A::HPCSparseMatrix{T,Ti,B}, Xr::ROCArray{Float64}, ldx::Int, m::Int, Q::Vector{Int}) where {T,Ti,B<:ROCBackend}
    # (raw pointers of X's rows and of the temporaries below go to queued kernels: every array stays referenced to the end)
    Base.GC.@preserve Xr _spmm_t_result_preserved(A, Xr, ldx, m, Q)
end
function _spmm_t_result_preserved(A::HPCSparseMatrix{T,Ti,B}, Xr::ROCArray{Float64}, ldx::Int, m::Int, Q::Vector{Int}) where {T,Ti,B<:ROCBackend}
    xp = A.nrows_local > 0 ? _ptr(Xr) : C_NULL
    comm = A.backend.comm
    nranks, rank = comm_size(comm), comm_rank(comm)
    n = A.col_partition[end] - 1
    st = _spmm_t_plan(A)
    if nranks == 1                     # W row-major over the (global) columns IS the column-major m x n block
        C = ROCMatrix{Float64}(undef, m, n)
        return _spmm_t_product!(C, A, st, xp, ldx, m)
    end
    W = ROCVector{Float64}(undef, max(st.n_split * m, 1))
    R = ROCVector{Float64}(undef, max(st.n_recv * m, 1))
    send = ROCVector{Float64}(undef, max(st.n_own * m, 1))
    C = ROCMatrix{Float64}(undef, Q[rank + 2] - Q[rank + 1], n)
    Base.GC.@preserve W R send C begin
    _spmm_t_product!(W, A, st, xp, ldx, m)
    if m > 0
        _ranges!(comm, W, R, st.back_ranks, st.back_off, st.back_cnt, st.from_ranks, st.from_off, st.from_cnt, 0, 0, 0, m)
        if st.acc !== nothing
            rows, ptr, pos, nu = st.acc
            _check(@ccall(LIB.hpcla_spmm_t_accumulate_f64(_ptr(W)::Ptr{Cvoid}, m::Int64, _ptr(R)::Ptr{Cvoid}, m::Int64,
                   _ptr(rows)::Ptr{Cvoid}, _ptr(ptr)::Ptr{Cvoid}, _ptr(pos)::Ptr{Cvoid}, nu::Int64, m::Int64,
                   _stream()::Ptr{Cvoid})::Cint), "hpcla_spmm_t_accumulate_f64")
        end
    end
    # V = W[1:n_own, :] (row-major, rows on A.col_partition): rank r gets V[:, Q_r] row-major, which is the column-major
    # (q_r x n_own) block at column A.col_partition[rank] of its result -- packed here, received in place
    P = A.col_partition
    q_me = Q[rank + 2] - Q[rank + 1]
    so, sc, sr = Int64[], Int64[], Int[]
    lsrc = 0
    for r in 0:nranks-1
        qr = Q[r + 2] - Q[r + 1]
        _place!(_ptr(W) + 8 * (Q[r + 1] - 1), m, _ptr(send) + 8 * st.n_own * (Q[r + 1] - 1), qr, st.n_own, qr)
        r == rank && (lsrc = st.n_own * (Q[r + 1] - 1))
        r != rank && qr * st.n_own > 0 && (push!(sr, r); push!(so, st.n_own * (Q[r + 1] - 1)); push!(sc, qr * st.n_own))
    end
    rr = [q for q in 0:nranks-1 if q != rank && q_me * (P[q + 2] - P[q + 1]) > 0]
    _ranges!(comm, send, C, sr, so, sc, rr, [q_me * (P[q + 1] - 1) for q in rr], [q_me * (P[q + 2] - P[q + 1]) for q in rr],
             lsrc, q_me * (P[rank + 1] - 1), q_me * st.n_own, 1)
    end
    return C
end

# a row-major block (width m) on the row partition PX, moved to the row partition PA: one range exchange, device to device
function _rows_on(comm, rows, PX::Vector{Int}, PA::Vector{Int}, m::Int)
    PX == PA && return rows
    nranks, rank = comm_size(comm), comm_rank(comm)
    out = ROCVector{Float64}(undef, max((PA[rank + 2] - PA[rank + 1]) * m, 1))
    ov(a, b) = (max(PX[a + 1], PA[b + 1]), min(PX[a + 2], PA[b + 2]))      # rows of X-rank a that A-rank b holds
    sr = [r for r in 0:nranks-1 if r != rank && ov(rank, r)[2] > ov(rank, r)[1]]
    rr = [q for q in 0:nranks-1 if q != rank && ov(q, rank)[2] > ov(q, rank)[1]]
    lo, hi = ov(rank, rank)
    _ranges!(comm, rows, out, sr, [ov(rank, r)[1] - PX[rank + 1] for r in sr], [ov(rank, r)[2] - ov(rank, r)[1] for r in sr],
             rr, [ov(q, rank)[1] - PA[rank + 1] for q in rr], [ov(q, rank)[2] - ov(q, rank)[1] for q in rr],
             max(lo - PX[rank + 1], 0), max(lo - PA[rank + 1], 0), max(hi - lo, 0), m)
    return out
end

function _dense_sparse_t(X::HPCMatrix{T,B}, A::HPCSparseMatrix{T,Ti,B}) where {T,Ti,B<:ROCBackend}
    assert_backends_compatible(X.backend, A.backend)
    X.row_partition[end] == A.row_partition[end] ||
        error("dimension mismatch: transpose(X) has $(X.row_partition[end] - 1) columns, A has $(A.row_partition[end] - 1) rows")
    nloc, m = size(X.A)
    rows = ROCVector{Float64}(undef, max(nloc * m, 1))          # the column-major block as rows (the kernel's layout)
    nloc > 0 && m > 0 && _check(@ccall(LIB.hpcla_transpose_f64(_ptr(X.A)::Ptr{Cvoid}, max(nloc, 1)::Int64, 1::Cint,
           _ptr(rows)::Ptr{Cvoid}, m::Int64, 0::Cint, nloc::Int64, m::Int64, _stream()::Ptr{Cvoid})::Cint), "hpcla_transpose_f64")
    C = Base.GC.@preserve rows begin
        aligned = _rows_on(A.backend.comm, rows, X.row_partition, A.row_partition, m)   # X on another row partition: device to device
        _spmm_t_result(A, aligned, max(m, 1), m, X.col_partition)
    end
    return HPCMatrix{T,B}(nothing, copy(X.col_partition),
                          HPCLinearAlgebra.uniform_partition(A.col_partition[end] - 1, comm_size(A.backend.comm)), C, A.backend)
end

function _dense_sparse(X::HPCMatrix{T,B}, A::HPCSparseMatrix{T,Ti,B}) where {T,Ti,B<:ROCBackend}
    assert_backends_compatible(X.backend, A.backend)
    mloc, p = size(X.A)
    p == A.row_partition[end] - 1 || error("dimension mismatch: X has $p columns, A has $(A.row_partition[end] - 1) rows")
    comm = A.backend.comm
    nranks, rank = comm_size(comm), comm_rank(comm)
    m = X.row_partition[end] - 1
    if nranks == 1                     # the column-major m x p block IS transpose(X) as rows (leading dimension m)
        C = _spmm_t_result(A, X.A, max(m, 1), m, X.row_partition)
    else
        # transpose(X) onto A's rows: X's column-major block is (p x mloc) row-major, rank r's rows are one range; the blocks
        # land side by side as rows of leading dimension m
        PA, PX = A.row_partition, X.row_partition
        nloc = A.nrows_local
        buf = ROCVector{Float64}(undef, max(nloc * m, 1))
        Xt = ROCVector{Float64}(undef, max(nloc * m, 1))
        rr = [q for q in 0:nranks-1 if q != rank && nloc * (PX[q + 2] - PX[q + 1]) > 0]
        sr = [r for r in 0:nranks-1 if r != rank && mloc * (PA[r + 2] - PA[r + 1]) > 0]
        Base.GC.@preserve buf Xt begin
        _ranges!(comm, X.A, buf, sr, [mloc * (PA[r + 1] - 1) for r in sr], [mloc * (PA[r + 2] - PA[r + 1]) for r in sr],
                 rr, [nloc * (PX[q + 1] - 1) for q in rr], [nloc * (PX[q + 2] - PX[q + 1]) for q in rr],
                 mloc * (PA[rank + 1] - 1), nloc * (PX[rank + 1] - 1), nloc * mloc, 1)
        for q in 0:nranks-1
            mq = PX[q + 2] - PX[q + 1]
            _place!(_ptr(buf) + 8 * nloc * (PX[q + 1] - 1), mq, _ptr(Xt) + 8 * (PX[q + 1] - 1), m, nloc, mq)
        end
        end
        C = _spmm_t_result(A, Xt, max(m, 1), m, X.row_partition)
    end
    return HPCMatrix{T,B}(nothing, copy(X.row_partition),
                          HPCLinearAlgebra.uniform_partition(A.col_partition[end] - 1, nranks), C, A.backend)
end
function Base.:*(M::HPCMatrix{Float64,B}, A::HPCSparseMatrix{Float64,Ti,B}) where {Ti,B<:ROCBackend}
    return _dense_sparse(M, A)
end
function Base.:*(Mt::Transpose{Float64,HPCMatrix{Float64,B}}, A::HPCSparseMatrix{Float64,Ti,B}) where {Ti,B<:ROCBackend}
    return _dense_sparse_t(LinearAlgebra.transpose(Mt), A)     # the transpose of a lazy transpose is its parent
end

end # module
