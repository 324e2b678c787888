# LDPCDecodersMI355X.jl -- Julia shim over libldpc_mi355x.so (include/ldpc_mi355x.h).
#
# NOT EXECUTED in this repository's pipeline: no Julia runtime exists in the build image
# or on the GPU box.  The same C ABI is exercised from Python ctypes
# (ldpcdecoders.jl_amd/_capi.py, decoder.py) and by the test-suite; this file is the
# binding a maintainer of QuantumSavory/LDPCDecoders.jl would add.  It mirrors
#
#   BeliefPropagationDecoder(H, per, max_iters)   src/decoders/belief_propagation.jl:61-67
#   reset!(decoder)                               :83-91
#   decode!(decoder, syndrome)                    :121-188
#   batchdecode!(decoder, syndromes, errors[, success])   :220-231, abstract_decoder.jl:44-48
#
# so that `MI355XBeliefPropagationDecoder <: LDPCDecoders.AbstractDecoder` is a drop-in
# wherever an AbstractDecoder is accepted (generic batchdecode!, QuantumClifford's extension).
# BP+OSD gets its own mirror type below (the reference's OSD decoder stores a concretely typed
# BeliefPropagationDecoder and reads `scratch.log_probabs`, belief_propagation_osd.jl:19,52).
module LDPCDecodersMI355X

using SparseArrays
import Libdl
import Random
import LDPCDecoders
import LDPCDecoders: AbstractDecoder, decode!, batchdecode!, reset!

export MI355XBeliefPropagationDecoder, MI355XBeliefPropagationOSDDecoder, MI355XBPOTSDecoder, MI355XBitFlipDecoder
export MI355XMinSumDecoder
export MI355XRelayDecoder
export Trials, sample!, score!, set_rates!, sample_rates!, sample_rates_device!
export CSSTrials

const libldpc = get(ENV, "LDPC_MI355X_LIB", "libldpc_mi355x.so")

const LDPC_OK = Cint(0)

struct LDPCMI355XError <: Exception
    status::Cint
    msg::String
end

function check(status::Cint)
    status == LDPC_OK && return nothing
    msg = unsafe_string(ccall((:ldpc_last_error, libldpc), Cstring, ()))
    # shape errors are assertion failures in the reference (belief_propagation.jl:221-222)
    status == 1 && throw(ArgumentError(msg))
    throw(LDPCMI355XError(status, msg))
end

"Host mirrors of the two scratch fields other code reads (belief_propagation.jl:3-18)."
struct MI355XScratch
    log_probabs::Vector{Float64}
    channel_probs::Vector{Float64}
    err::Vector{Float64}
end

mutable struct MI355XBeliefPropagationDecoder <: AbstractDecoder
    per::Float64
    max_iters::Int
    s::Int
    n::Int
    sparse_H::SparseMatrixCSC{Bool,Int}
    sparse_HT::SparseMatrixCSC{Bool,Int}
    scratch::MI355XScratch
    handle::Ptr{Cvoid}       # ldpc_bp_decoder* (with `devices`: the root's, owned by `multi`)
    multi::Ptr{Cvoid}        # ldpc_bp_multi* when the decoder partitions its batches over several GPUs, else C_NULL
    # reusable staging (column-major Julia matrices already have the ABI's [B][s] image)
    syn_u8::Vector{UInt8}
    err_u8::Vector{UInt8}
    conv_u8::Vector{UInt8}
    syn_bits::BitVector      # reusable packed images for the bits entry (bit_io.jl)
    err_bits::BitVector
end

"""
    MI355XBeliefPropagationDecoder(H, per, max_iters; device=-1, devices=nothing, exchange=0, llr_exact=false)

`llr_exact = true`: `scratch.log_probabs` from the full posterior odds (`ldpc_bp_options.llr_exact`; the default cuts the odds
to their upper 32 bits: LLRs within 5e-7 of the reference's).  The BP+OSD type below asks for it.

`devices = 0:7` makes `batchdecode!` one call that partitions the columns of its `syndromes` matrix over those GPUs
(`ldpc_bp_create_multi`: contiguous shards, one handle and stream per GPU; the host arrays go pinned host -> each
shard's own GPU and back).  `exchange` only matters for device-resident batches (`ldpc_bp_decode_batch_multi_device`:
0 auto = RCCL send/recv from `devices[1]`, 1 hipMemcpyPeer, 2 RCCL).
"""
function MI355XBeliefPropagationDecoder(H, per::Float64, max_iters::Int; device::Integer=-1,
                                        devices::Union{Nothing,AbstractVector{<:Integer}}=nothing, exchange::Integer=0,
                                        llr_exact::Bool=false)
    s, n = size(H)
    sparse_H = SparseMatrixCSC{Bool,Int}(sparse(H))          # :63
    sparse_HT = SparseMatrixCSC{Bool,Int}(sparse(H'))        # :64
    colptr = Int64.(sparse_H.colptr .- 1)                    # zero-based for the ABI
    rowval = Int64.(rowvals(sparse_H) .- 1)
    opts = zeros(Int32, 16); opts[1] = Int32(device)         # ldpc_bp_options: device, waves_per_tile, resident_tiles,
    opts[6] = Int32(llr_exact)                               # kernel_variant, defer_threshold, llr_exact, reserved[10]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    m = C_NULL
    if devices === nothing
        check(ccall((:ldpc_bp_create, libldpc), Cint,
                    (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Float64, Int64, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                    s, n, length(rowval), colptr, rowval, per, max_iters, opts, h))
    else
        devs = Int32.(collect(devices))
        mr = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ldpc_bp_create_multi, libldpc), Cint,
                    (Int32, Ptr{Int32}, Int32, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Float64, Int64, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                    length(devs), devs, exchange, s, n, length(rowval), colptr, rowval, per, max_iters, opts, mr))
        m = mr[]
        h[] = ccall((:ldpc_bp_multi_handle, libldpc), Ptr{Cvoid}, (Ptr{Cvoid}, Int32), m, 0)
    end
    d = MI355XBeliefPropagationDecoder(per, max_iters, s, n, sparse_H, sparse_HT,
            MI355XScratch(zeros(n), fill(per, n), zeros(n)), h[], m, UInt8[], UInt8[], UInt8[], BitVector(), BitVector())
    finalizer(d) do x
        if x.multi != C_NULL
            ccall((:ldpc_bp_destroy_multi, libldpc), Cint, (Ptr{Cvoid},), x.multi)   # (owns every per-GPU handle)
        elseif x.handle != C_NULL
            ccall((:ldpc_bp_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        end
        x.handle = C_NULL; x.multi = C_NULL
    end
    return d
end

# the host-buffer entry: one GPU, or the batch partitioned over `devices` (same argument list, belief_propagation.jl:220-231)
host_decode(d::MI355XBeliefPropagationDecoder, B, llr) = d.multi != C_NULL ?
    ccall((:ldpc_bp_decode_batch_multi, libldpc), Cint,
          (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
          d.multi, B, d.syn_u8, d.err_u8, d.conv_u8, llr, C_NULL) :
    ccall((:ldpc_bp_decode_batch, libldpc), Cint,
          (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
          d.handle, B, d.syn_u8, d.err_u8, d.conv_u8, llr, C_NULL)

"""
    last_status(d)

Waits for everything enqueued on the handle and throws if a team of workgroups lost a member in one of
those calls (`ldpc_bp_last_status`, include/ldpc_mi355x.h).  Only callers of the asynchronous device entry
need it; `decode!` / `batchdecode!` above use the synchronous host entry, which repairs such a call itself.
"""
last_status(d::MI355XBeliefPropagationDecoder) = d.multi != C_NULL ?
    check(ccall((:ldpc_bp_multi_last_status, libldpc), Cint, (Ptr{Cvoid},), d.multi)) :
    check(ccall((:ldpc_bp_last_status, libldpc), Cint, (Ptr{Cvoid},), d.handle))

"`(-1)^x` only needs the parity; anything but 0/1 must never match the convergence `==` (:136,:181)."
@inline function syndrome_byte(x)::UInt8
    v = Int(x)                      # InexactError for non-integral floats, like (-1)^2.5 -> DomainError
    (v == 0 || v == 1) ? UInt8(v) : UInt8(2 + (v & 1))
end

function reset!(d::MI355XBeliefPropagationDecoder)            # :83-91 (device scratch is reset per call)
    d.scratch.log_probabs .= 0.0
    d.scratch.channel_probs .= d.per
    d.scratch.err .= 0.0
    d
end

function decode!(d::MI355XBeliefPropagationDecoder, syndrome::AbstractVector)   # :121-188
    length(syndrome) == d.s || throw(BoundsError(syndrome, d.s))
    reset!(d)
    resize!(d.syn_u8, d.s); resize!(d.err_u8, d.n); resize!(d.conv_u8, 1)
    @inbounds for i in 1:d.s
        d.syn_u8[i] = syndrome_byte(syndrome[i])
    end
    check(host_decode(d, 1, d.scratch.log_probabs))
    @inbounds for j in 1:d.n
        d.scratch.err[j] = d.err_u8[j]
    end
    return d.scratch.err, d.conv_u8[1] != 0                   # alias of the scratch, like :187
end

# the two host entries on explicit pointers (bit_io.jl chooses between them by the argument types)
bytes_call(d::MI355XBeliefPropagationDecoder, B, syn, err, conv, llr) = d.multi != C_NULL ?
    ccall((:ldpc_bp_decode_batch_multi, libldpc), Cint,
          (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
          d.multi, B, syn, err, conv, llr, C_NULL) :
    ccall((:ldpc_bp_decode_batch, libldpc), Cint,
          (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
          d.handle, B, syn, err, conv, llr, C_NULL)
bits_call(d::MI355XBeliefPropagationDecoder, B, synw, sbit0, errw, ebit0, conv, llr) = d.multi != C_NULL ?
    ccall((:ldpc_bp_decode_batch_multi_bits, libldpc), Cint,
          (Ptr{Cvoid}, Int64, Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
          d.multi, B, synw, sbit0, errw, ebit0, conv, llr, C_NULL) :
    ccall((:ldpc_bp_decode_batch_bits, libldpc), Cint,
          (Ptr{Cvoid}, Int64, Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
          d.handle, B, synw, sbit0, errw, ebit0, conv, llr, C_NULL)

include(joinpath(@__DIR__, "bit_io.jl"))

function batchdecode!(d::MI355XBeliefPropagationDecoder, syndromes::AbstractMatrix,
                      errors::AbstractMatrix, success::AbstractVector{Bool})   # :220-231
    @assert size(syndromes, 2) == size(errors, 2)             # :221
    @assert size(syndromes, 2) == length(success)             # :222
    B = size(syndromes, 2)
    size(syndromes, 1) == d.s || throw(DimensionMismatch("syndromes has $(size(syndromes,1)) rows, decoder has $(d.s) checks"))
    size(errors, 1) == d.n || throw(DimensionMismatch("errors has $(size(errors,1)) rows, decoder has $(d.n) bits"))
    B == 0 && return errors, success
    # one call, one matrix -- on one GPU or partitioned over `devices`.  BitMatrix arguments go to the bits entry in
    # place, Matrix{UInt8} / Matrix{Bool} to the byte entry in place, anything else is packed once (bit_io.jl)
    marshal_batchdecode!(d, d.s, d.n, syndromes, errors, success)
    # the reference's per-column loop (:224-228) leaves the scratch with the LAST column's decision and LLRs: that
    # column is decoded once more alone (deterministic per syndrome)
    last_column!(d, d.s, d.n, syndromes, d.scratch.err, d.scratch.log_probabs)
    return errors, success                                    # :230
end

# 3-argument form: the generic method at abstract_decoder.jl:44-48 allocates `success`
# and re-dispatches to the 4-argument method above; nothing to add.

# ---------------------------------------------------------------------------------------------
# BP+OSD (src/decoders/belief_propagation_osd.jl).  The reference's BeliefPropagationOSDDecoder
# holds a concretely typed `bp_decoder::BeliefPropagationDecoder` (:19), so the MI355X decoder
# cannot be slotted into it; this type mirrors it: BP on the GPU, the ordered-statistics step in
# the library's host code (`ldpc_osd_postprocess_batch`, bit-packed, threaded over the batch).
# ---------------------------------------------------------------------------------------------
mutable struct MI355XBeliefPropagationOSDDecoder <: AbstractDecoder
    bp_decoder::MI355XBeliefPropagationDecoder
    H::BitMatrix
    osd_order::Int
    osd_handle::Ptr{Cvoid}
end

function MI355XBeliefPropagationOSDDecoder(H::BitMatrix, per::Float64, max_iters::Int;
                                           osd_order::Int=0, device::Integer=-1)     # :26-29
    bp = MI355XBeliefPropagationDecoder(H, per, max_iters; device=device, llr_exact=true)   # (OSD orders bits by reliability, :53-55)
    colptr = Int64.(bp.sparse_H.colptr .- 1); rowval = Int64.(rowvals(bp.sparse_H) .- 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ldpc_osd_create, libldpc), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Ptr{Cvoid}}),
                bp.s, bp.n, length(rowval), colptr, rowval, osd_order, h))
    d = MI355XBeliefPropagationOSDDecoder(bp, H, osd_order, h[])
    finalizer(d) do x
        x.osd_handle != C_NULL && ccall((:ldpc_osd_destroy, libldpc), Cint, (Ptr{Cvoid},), x.osd_handle)
        x.osd_handle = C_NULL
    end
    return d
end

function decode!(d::MI355XBeliefPropagationOSDDecoder, syndrome::AbstractVector)      # :49-61
    bp = d.bp_decoder
    bp_err, converged = decode!(bp, syndrome)              # fills bp.syn_u8, bp.err_u8, scratch.log_probabs
    out = Vector{UInt8}(undef, bp.n)
    check(ccall((:ldpc_osd_postprocess_batch, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{UInt8}, Int32),
                d.osd_handle, 1, bp.syn_u8, bp.err_u8, bp.scratch.log_probabs, out, 1))
    return Bool.(out), converged                           # a Bool vector, like :60
end

function batchdecode!(d::MI355XBeliefPropagationOSDDecoder, syndromes::AbstractMatrix,
                      errors::AbstractMatrix, success::AbstractVector{Bool})
    # one BP launch + one threaded OSD pass give the same columns as the reference's generic
    # per-column loop (abstract_decoder.jl:31-42, test_bposd_decoder.jl:49-57)
    @assert size(syndromes, 2) == size(errors, 2)
    @assert size(syndromes, 2) == length(success)
    bp = d.bp_decoder
    B = size(syndromes, 2)
    B == 0 && return errors, success
    resize!(bp.syn_u8, bp.s * B); resize!(bp.err_u8, bp.n * B); resize!(bp.conv_u8, B)
    @inbounds for i in 1:B, r in 1:bp.s
        bp.syn_u8[(i - 1) * bp.s + r] = syndrome_byte(syndromes[r, i])
    end
    llr = Vector{Float64}(undef, bp.n * B)
    check(host_decode(bp, B, llr))
    out = Vector{UInt8}(undef, bp.n * B)
    check(ccall((:ldpc_osd_postprocess_batch, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{UInt8}, Int32),
                d.osd_handle, B, bp.syn_u8, bp.err_u8, llr, out, 0))
    @inbounds for i in 1:B
        success[i] = bp.conv_u8[i] != 0
        for j in 1:bp.n
            errors[j, i] = out[(i - 1) * bp.n + j]
        end
    end
    return errors, success
end

# The opt-in DEVICE form of the ordered-statistics step (include/ldpc_mi355x.h: its stated reliability key, the tiers).
# For callers that keep their batches on the GPU (AMDGPU.jl arrays, or pointers obtained elsewhere): prepare once, then
# hand device pointers and a hipStream_t; `d_errors` may be `d_bp_errors` itself.
osd_device_prepare!(d::MI355XBeliefPropagationOSDDecoder; device::Integer=-1, kernel_variant::Integer=0) =
    check(ccall((:ldpc_osd_device_prepare, libldpc), Cint, (Ptr{Cvoid}, Int32, Int32), d.osd_handle, device, kernel_variant))

osd_device_kernel(d::MI355XBeliefPropagationOSDDecoder) =
    Int(ccall((:ldpc_osd_device_kernel, libldpc), Int32, (Ptr{Cvoid},), d.osd_handle))

function osd_postprocess_device!(d::MI355XBeliefPropagationOSDDecoder, batch::Integer, d_syndromes::Ptr{UInt8},
                                 d_bp_errors::Ptr{UInt8}, d_llr::Ptr{Float64}, d_errors::Ptr{UInt8},
                                 stream::Ptr{Cvoid}=C_NULL)
    check(ccall((:ldpc_osd_postprocess_batch_device, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{UInt8}, Ptr{Cvoid}),
                d.osd_handle, batch, d_syndromes, d_bp_errors, d_llr, d_errors, stream))
    return nothing
end

# The standard rule of the ordered-statistics step (include/ldpc_mi355x.h "THE STANDARD RULE"; device form only): call
# before osd_device_prepare!.  method 0 = the reference rule, 1 = exhaustive, 2 = combination sweep; channel_llr = nothing
# weighs by count.
function osd_set_search!(d::MI355XBeliefPropagationOSDDecoder, method::Integer, order::Integer,
                         channel_llr::Union{Nothing,Vector{Float64}}=nothing)
    n = size(d.H, 2)
    check(ccall((:ldpc_osd_set_search, libldpc), Cint, (Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Float64}),
                d.osd_handle, method, order, n, channel_llr === nothing ? Ptr{Float64}(C_NULL) : pointer(channel_llr)))
    return nothing
end

osd_search_method(d::MI355XBeliefPropagationOSDDecoder) =
    Int(ccall((:ldpc_osd_search_method, libldpc), Int32, (Ptr{Cvoid},), d.osd_handle))

osd_search_weight(d::MI355XBeliefPropagationOSDDecoder, j::Integer) =
    ccall((:ldpc_osd_search_weight, libldpc), Int64, (Ptr{Cvoid}, Int64), d.osd_handle, j)

# ---------------------------------------------------------------------------------------------
# BP-OTS (src/decoders/bpots_decoder.jl:39-115, 225-340) over ldpc_bpots_* (LDS-resident kernel for small graphs,
# node-parallel kernel with the messages in global memory up to n ~ 30,000; beyond that LDPCMI355XError(5, ...)).
# ---------------------------------------------------------------------------------------------
mutable struct MI355XBPOTSDecoder <: AbstractDecoder
    per::Float64; max_iters::Int; s::Int; n::Int; T::Int; C::Float64
    handle::Ptr{Cvoid}
end

function MI355XBPOTSDecoder(H::Union{SparseMatrixCSC{Bool,Int},BitMatrix}, per::Float64, max_iters::Int;
                            T::Int=9, C::Float64=2.0, device::Integer=-1)             # :90
    s, n = size(H)
    sp = SparseMatrixCSC{Bool,Int}(sparse(H))
    colptr = Int64.(sp.colptr .- 1); rowval = Int64.(rowvals(sp) .- 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ldpc_bpots_create, libldpc), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Float64, Int64, Int64, Float64, Int32, Ptr{Ptr{Cvoid}}),
                s, n, length(rowval), colptr, rowval, per, max_iters, T, C, device, h))
    d = MI355XBPOTSDecoder(per, max_iters, s, n, T, C, h[])
    finalizer(d) do x
        x.handle != C_NULL && ccall((:ldpc_bpots_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        x.handle = C_NULL
    end
    return d
end

reset!(d::MI355XBPOTSDecoder) = d       # :142-154: the device state is reset inside every decode call

function decode!(d::MI355XBPOTSDecoder, syndrome::AbstractVector)                      # :225-340
    length(syndrome) == d.s || throw(BoundsError(syndrome, d.s))
    syn = UInt8[syndrome_byte(x) for x in syndrome]
    err = Vector{UInt8}(undef, d.n); conv = Vector{UInt8}(undef, 1)
    check(ccall((:ldpc_bpots_decode_batch, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}),
                d.handle, 1, syn, err, conv, C_NULL))
    return Int.(err), conv[1] != 0        # best_decisions::Vector{Int}, converged
end
# batchdecode! on it is the reference's generic per-column method (abstract_decoder.jl:31-48);
# a batched override would call ldpc_bpots_decode_batch with B columns exactly like the BP type above.

# ---------------------------------------------------------------------------------------------
# Bit flip (src/decoders/iterative_bitflip.jl:61-68, 116-201) over ldpc_bitflip_*.  The reference breaks ties among the
# bits with the largest vote with `rand`; the library's tie rule (include/ldpc_mi355x.h) is a function of (seed, column
# number, iteration): the decoder numbers the columns it decodes (`columns_decoded`), so repeated decode! calls on one
# syndrome draw fresh tie-breaks and a fixed seed replays a session.
# ---------------------------------------------------------------------------------------------
mutable struct MI355XBitFlipDecoder <: AbstractDecoder
    per::Float64; max_iters::Int; s::Int; n::Int
    sparse_H::SparseMatrixCSC{Bool,Int}
    err::Vector{Int}
    columns_decoded::Int64
    handle::Ptr{Cvoid}
end

"ldpc_bitflip_options: int32 device, int32 tie_break, uint64 seed, int32 kernel_variant, int32 reserved[11] (64 bytes)"
function bitflip_options(device::Integer, tie_break::Integer, seed::Integer, kernel_variant::Integer)
    opts = zeros(Int32, 16)
    opts[1] = Int32(device); opts[2] = Int32(tie_break); opts[5] = Int32(kernel_variant)
    sd = UInt64(seed)
    opts[3] = reinterpret(Int32, UInt32(sd & 0xffffffff)); opts[4] = reinterpret(Int32, UInt32(sd >> 32))   # little-endian
    return opts
end

"""
    MI355XBitFlipDecoder(H, per, max_iters; tie_break=0, seed=0, device=-1, kernel_variant=0)

`tie_break`: 0 random (seeded), 1 first, 2 last candidate in ascending bit order.
"""
function MI355XBitFlipDecoder(H, per::Float64, max_iters::Int; tie_break::Integer=0, seed::Integer=0,
                              device::Integer=-1, kernel_variant::Integer=0)
    s, n = size(H)
    sp = dropzeros(SparseMatrixCSC{Bool,Int}(sparse(H)))      # only `true` entries count (`sparse_H[i, j]`, :135)
    colptr = Int64.(sp.colptr .- 1); rowval = Int64.(rowvals(sp) .- 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ldpc_bitflip_create, libldpc), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Float64, Int64, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                s, n, length(rowval), colptr, rowval, per, max_iters, bitflip_options(device, tie_break, seed, kernel_variant), h))
    d = MI355XBitFlipDecoder(per, max_iters, s, n, sp, zeros(Int, n), 0, h[])
    finalizer(d) do x
        x.handle != C_NULL && ccall((:ldpc_bitflip_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        x.handle = C_NULL
    end
    return d
end

reset!(d::MI355XBitFlipDecoder) = d     # :84-88: the device state is reset inside every decode call

bitflip_call(handle, B, column0, syn, err, conv) =
    check(ccall((:ldpc_bitflip_decode_batch, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}, Ptr{UInt8}),
                handle, B, column0, syn, err, conv, C_NULL, C_NULL))

function decode!(d::MI355XBitFlipDecoder, syndrome::AbstractVector)                    # :116-157
    length(syndrome) == d.s || throw(BoundsError(syndrome, d.s))
    syn = UInt8[syndrome_byte(x) for x in syndrome]
    err = Vector{UInt8}(undef, d.n); conv = Vector{UInt8}(undef, 1)
    bitflip_call(d.handle, 1, d.columns_decoded, syn, err, conv)
    d.columns_decoded += 1
    d.err .= err
    return d.err, conv[1] != 0            # (setup.err, converged)
end

# 0/1 bytes already: Matrix{UInt8} and Matrix{Bool} are the ABI's [B][s] image and go through without a conversion loop
bitflip_image(syndromes::Matrix{UInt8}) = all(x -> x <= 0x01, syndromes) ? syndromes : map(syndrome_byte, syndromes)
bitflip_image(syndromes::Matrix{Bool}) = reinterpret(UInt8, syndromes)
bitflip_image(syndromes::AbstractMatrix) = UInt8[syndrome_byte(x) for x in syndromes]

function batchdecode!(d::MI355XBitFlipDecoder, syndromes::AbstractMatrix, errors::AbstractMatrix,
                      converged::AbstractVector{Bool})                                 # :189-201, one device call
    @assert size(syndromes, 2) == size(errors, 2)
    @assert size(syndromes, 2) == length(converged)
    size(syndromes, 1) == d.s && size(errors, 1) == d.n || throw(DimensionMismatch("syndromes / errors rows"))
    B = size(syndromes, 2)
    B == 0 && return errors, converged
    direct = errors isa Matrix{UInt8} || errors isa Matrix{Bool}
    err = direct ? reinterpret(UInt8, errors) : Matrix{UInt8}(undef, d.n, B)
    conv = Vector{UInt8}(undef, B)
    bitflip_call(d.handle, B, d.columns_decoded, bitflip_image(syndromes), err, conv)
    d.columns_decoded += B
    direct || (errors .= err)
    converged .= conv .!= 0
    d.err .= view(err, :, B)
    return errors, converged
end
batchdecode!(d::MI355XBitFlipDecoder, syndromes::AbstractMatrix, errors::AbstractMatrix) =
    batchdecode!(d, syndromes, errors, Vector{Bool}(undef, size(syndromes, 2)))

# ---------------------------------------------------------------------------------------------
# Normalised min-sum with one channel LLR per bit over ldpc_minsum_* (not a decoder of the reference; the rule is stated
# in include/ldpc_mi355x.h).  The library computes no logarithm: the Float32 prior LLRs log((1 - p) / p) are formed here.
# These symbols were added without a change of the ABI version; look them up with Libdl.dlsym as for the trials entries.
# ---------------------------------------------------------------------------------------------
mutable struct MI355XMinSumDecoder <: AbstractDecoder
    per::Union{Float64,Nothing}; max_iters::Int; s::Int; n::Int
    sparse_H::SparseMatrixCSC{Bool,Int}
    channel_llr::Vector{Float32}
    err::Vector{Float64}
    log_probabs::Vector{Float64}
    handle::Ptr{Cvoid}
end

"ldpc_minsum_options: int32 device, float alpha, float clip, int32 kernel_variant, int32 schedule (0 = flooding, 1 = layered), int32 reserved[11] (64 bytes)"
function minsum_options(device::Integer, alpha::Real, clip::Real, kernel_variant::Integer, schedule::Integer=0)
    opts = zeros(Int32, 16)
    opts[1] = Int32(device); opts[4] = Int32(kernel_variant); opts[5] = Int32(schedule)
    opts[2] = reinterpret(Int32, Float32(alpha)); opts[3] = reinterpret(Int32, Float32(clip))
    return opts
end

minsum_llr(p) = Float32(log((1.0 - Float64(p)) / Float64(p)))

"""
    MI355XMinSumDecoder(H, per, max_iters; alpha=0.75, clip=1e6, device=-1, kernel_variant=0, schedule=:flooding)
    MI355XMinSumDecoder(H, max_iters; channel_probs=..., ...)   or   channel_llr=...

One prior per bit: a uniform `per`, error probabilities strictly inside (0, 1), or finite LLRs log(P(0) / P(1)).
`schedule`: `:flooding`, or `:layered` (a check reads the posteriors the checks before it have just updated: THE
LAYERED RULE of include/ldpc_mi355x.h; `minsum_layers(d)` tells the number of layers); anything else is an ArgumentError.
"""
function MI355XMinSumDecoder(H, per::Union{Float64,Nothing}, max_iters::Int; channel_probs=nothing, channel_llr=nothing,
                             alpha::Real=0.75, clip::Real=1e6, device::Integer=-1, kernel_variant::Integer=0,
                             schedule::Symbol=:flooding)
    s, n = size(H)
    schedule in (:flooding, :layered) || throw(ArgumentError("schedule must be :flooding or :layered"))
    count(!isnothing, (per, channel_probs, channel_llr)) == 1 ||
        throw(ArgumentError("give exactly one of per, channel_probs and channel_llr"))
    probs = per !== nothing ? fill(per, n) : channel_probs
    probs === nothing || all(p -> 0 < p < 1, probs) || throw(DomainError(probs, "probabilities must lie strictly inside (0, 1)"))
    llr = probs !== nothing ? Float32[minsum_llr(p) for p in probs] : Vector{Float32}(channel_llr)
    length(llr) == n || throw(DimensionMismatch("one prior per bit"))
    (Float32(alpha) == 0 || Float32(clip) == 0) && throw(ArgumentError("alpha and clip must not be zero"))   # (0 = default in the C struct)
    sp = dropzeros(SparseMatrixCSC{Bool,Int}(sparse(H)))
    colptr = Int64.(sp.colptr .- 1); rowval = Int64.(rowvals(sp) .- 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ldpc_minsum_create, libldpc), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float32}, Int64, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                s, n, length(rowval), colptr, rowval, llr, max_iters, minsum_options(device, alpha, clip, kernel_variant, schedule === :layered ? 1 : 0), h))
    d = MI355XMinSumDecoder(per, max_iters, s, n, sp, llr, zeros(n), zeros(n), h[])
    finalizer(d) do x
        x.handle != C_NULL && ccall((:ldpc_minsum_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        x.handle = C_NULL
    end
    return d
end
MI355XMinSumDecoder(H, max_iters::Int; kwargs...) = MI355XMinSumDecoder(H, nothing, max_iters; kwargs...)

reset!(d::MI355XMinSumDecoder) = d      # the device state is reset inside every decode call
"the number of layers of a layered handle, 0 for the flooding schedule (ldpc_minsum_layers)"
minsum_layers(d::MI355XMinSumDecoder) = Int(ccall((:ldpc_minsum_layers, libldpc), Int32, (Ptr{Cvoid},), d.handle))

minsum_call(handle, B, syn, err, conv, llr) =
    check(ccall((:ldpc_minsum_decode_batch, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                handle, B, syn, err, conv, llr, C_NULL))

# Per-syndrome priors (PER-SYNDROME PRIORS of include/ldpc_mi355x.h): host entries; the batch arrays are column-major
# n x B / s x B matrices, which is the library's [batch][n] layout.
"tier and S of the entries with per-syndrome priors (0, 0: unsupported on this handle)"
minsum_priors_plan(d::MI355XMinSumDecoder) =
    (Int(ccall((:ldpc_minsum_priors_kernel, libldpc), Int32, (Ptr{Cvoid},), d.handle)),
     Int(ccall((:ldpc_minsum_priors_tile_syndromes, libldpc), Int32, (Ptr{Cvoid},), d.handle)))

"syndromes s x B UInt8, priors n x B Float32 (one prior LLR per syndrome and bit) -> (errors n x B UInt8, converged)"
function minsum_decode_priors(d::MI355XMinSumDecoder, syndromes::Matrix{UInt8}, priors::Matrix{Float32})
    B = size(syndromes, 2)
    size(syndromes, 1) == d.s && size(priors) == (d.n, B) || throw(DimensionMismatch("syndromes / priors"))
    err = Matrix{UInt8}(undef, d.n, B); conv = Vector{UInt8}(undef, B)
    check(ccall((:ldpc_minsum_decode_batch_priors, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{Float32}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                d.handle, B, syndromes, priors, err, conv, C_NULL, C_NULL))
    return err, conv .!= 0
end

"the two tables of the given-bits entry: the prior LLR of every bit where its given bit is 0 / 1 (finite)"
function minsum_set_conditional_priors!(d::MI355XMinSumDecoder, llr_if0::Vector{Float32}, llr_if1::Vector{Float32})
    length(llr_if0) == d.n && length(llr_if1) == d.n || throw(DimensionMismatch("one entry per bit"))
    check(ccall((:ldpc_minsum_set_conditional_priors, libldpc), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}),
                d.handle, llr_if0, llr_if1))
    return d
end

"syndromes s x B UInt8, given n x B UInt8 (the low bit selects llr_if1 over llr_if0) -> (errors n x B UInt8, converged)"
function minsum_decode_given(d::MI355XMinSumDecoder, syndromes::Matrix{UInt8}, given::Matrix{UInt8})
    B = size(syndromes, 2)
    size(syndromes, 1) == d.s && size(given) == (d.n, B) || throw(DimensionMismatch("syndromes / given"))
    err = Matrix{UInt8}(undef, d.n, B); conv = Vector{UInt8}(undef, B)
    check(ccall((:ldpc_minsum_decode_batch_given, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                d.handle, B, syndromes, given, err, conv, C_NULL, C_NULL))
    return err, conv .!= 0
end

function decode!(d::MI355XMinSumDecoder, syndrome::AbstractVector)
    length(syndrome) == d.s || throw(BoundsError(syndrome, d.s))
    syn = UInt8[syndrome_byte(x) for x in syndrome]
    err = Vector{UInt8}(undef, d.n); conv = Vector{UInt8}(undef, 1)
    minsum_call(d.handle, 1, syn, err, conv, d.log_probabs)
    d.err .= err
    return d.err, conv[1] != 0
end

function batchdecode!(d::MI355XMinSumDecoder, syndromes::AbstractMatrix, errors::AbstractMatrix,
                      converged::AbstractVector{Bool})                                 # one device call
    @assert size(syndromes, 2) == size(errors, 2)
    @assert size(syndromes, 2) == length(converged)
    size(syndromes, 1) == d.s && size(errors, 1) == d.n || throw(DimensionMismatch("syndromes / errors rows"))
    B = size(syndromes, 2)
    B == 0 && return errors, converged
    direct = errors isa Matrix{UInt8} || errors isa Matrix{Bool}
    err = direct ? reinterpret(UInt8, errors) : Matrix{UInt8}(undef, d.n, B)
    conv = Vector{UInt8}(undef, B)
    minsum_call(d.handle, B, bitflip_image(syndromes), err, conv, C_NULL)
    direct || (errors .= err)
    converged .= conv .!= 0
    d.err .= view(err, :, B)
    return errors, converged
end
batchdecode!(d::MI355XMinSumDecoder, syndromes::AbstractMatrix, errors::AbstractMatrix) =
    batchdecode!(d, syndromes, errors, Vector{Bool}(undef, size(syndromes, 2)))

# ---------------------------------------------------------------------------------------------
# Relay min-sum over ldpc_relay_* (not a decoder of the reference; the rule is stated in include/ldpc_mi355x.h): min-sum
# with a per-bit memory strength gamma, run as a chain of legs, the lightest of the first `stop_after` solutions returned.
# The library draws no random number: the gammas are formed here.  Symbols added without a change of the ABI version.
# ---------------------------------------------------------------------------------------------
mutable struct MI355XRelayDecoder <: AbstractDecoder
    per::Union{Float64,Nothing}; max_iters::Int; s::Int; n::Int
    sparse_H::SparseMatrixCSC{Bool,Int}
    channel_llr::Vector{Float32}
    gammas::Matrix{Float32}          # n x legs: column r is leg r (the C array [legs][n])
    leg_iters::Vector{Int32}
    err::Vector{Float64}
    log_probabs::Vector{Float64}
    handle::Ptr{Cvoid}
end

"ldpc_relay_options: int32 device, float alpha, float clip, int32 kernel_variant, int32 stop_after, int32 reserved[11] (64 bytes)"
function relay_options(device::Integer, alpha::Real, clip::Real, kernel_variant::Integer, stop_after::Integer)
    opts = minsum_options(device, alpha, clip, kernel_variant)
    opts[5] = Int32(stop_after)
    return opts
end

"""
    MI355XRelayDecoder(H, per, max_iters; legs=9, leg_iters=20, gamma0=0.125, gamma_range=(-0.24, 0.66), gammas=nothing,
                       rng=Random.default_rng(), stop_after=1, alpha=0.75, clip=1e6, device=-1, kernel_variant=0)
    MI355XRelayDecoder(H, max_iters; channel_probs=..., ...)   or   channel_llr=...

Leg 0 runs `max_iters` iterations with `gamma0` everywhere, every later leg `leg_iters` with gammas drawn uniformly in
`gamma_range`; `gammas` (n x legs, each inside (-1, 1)) gives them outright.
"""
function MI355XRelayDecoder(H, per::Union{Float64,Nothing}, max_iters::Int; channel_probs=nothing, channel_llr=nothing,
                            legs::Int=9, leg_iters::Int=20, gamma0::Real=0.125, gamma_range=(-0.24, 0.66), gammas=nothing,
                            rng=Random.default_rng(), stop_after::Int=1, alpha::Real=0.75, clip::Real=1e6,
                            device::Integer=-1, kernel_variant::Integer=0)
    s, n = size(H)
    count(!isnothing, (per, channel_probs, channel_llr)) == 1 ||
        throw(ArgumentError("give exactly one of per, channel_probs and channel_llr"))
    legs >= 1 && stop_after >= 1 || throw(ArgumentError("legs and stop_after must be >= 1"))
    probs = per !== nothing ? fill(per, n) : channel_probs
    probs === nothing || all(p -> 0 < p < 1, probs) || throw(DomainError(probs, "probabilities must lie strictly inside (0, 1)"))
    llr = probs !== nothing ? Float32[minsum_llr(p) for p in probs] : Vector{Float32}(channel_llr)
    length(llr) == n || throw(DimensionMismatch("one prior per bit"))
    (Float32(alpha) == 0 || Float32(clip) == 0) && throw(ArgumentError("alpha and clip must not be zero"))   # (0 = default in the C struct)
    g = if gammas !== nothing
        Matrix{Float32}(gammas)
    else
        lo, hi = Float64.(gamma_range)
        hcat(fill(Float32(gamma0), n, 1), Float32.(lo .+ (hi - lo) .* rand(rng, n, legs - 1)))
    end
    size(g) == (n, legs) || throw(DimensionMismatch("gammas must be n x legs"))
    its = Int32[max_iters; fill(leg_iters, legs - 1)]
    sp = dropzeros(SparseMatrixCSC{Bool,Int}(sparse(H)))
    colptr = Int64.(sp.colptr .- 1); rowval = Int64.(rowvals(sp) .- 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ldpc_relay_create, libldpc), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                s, n, length(rowval), colptr, rowval, llr, legs, g, its, relay_options(device, alpha, clip, kernel_variant, stop_after), h))
    d = MI355XRelayDecoder(per, max_iters, s, n, sp, llr, g, its, zeros(n), zeros(n), h[])
    finalizer(d) do x
        x.handle != C_NULL && ccall((:ldpc_relay_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        x.handle = C_NULL
    end
    return d
end
MI355XRelayDecoder(H, max_iters::Int; kwargs...) = MI355XRelayDecoder(H, nothing, max_iters; kwargs...)

reset!(d::MI355XRelayDecoder) = d      # the device state is reset inside every decode call

relay_call(handle, B, syn, err, conv, llr) =
    check(ccall((:ldpc_relay_decode_batch, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                handle, B, syn, err, conv, llr, C_NULL, C_NULL))

function decode!(d::MI355XRelayDecoder, syndrome::AbstractVector)
    length(syndrome) == d.s || throw(BoundsError(syndrome, d.s))
    syn = UInt8[syndrome_byte(x) for x in syndrome]
    err = Vector{UInt8}(undef, d.n); conv = Vector{UInt8}(undef, 1)
    relay_call(d.handle, 1, syn, err, conv, d.log_probabs)
    d.err .= err
    return d.err, conv[1] != 0
end

function batchdecode!(d::MI355XRelayDecoder, syndromes::AbstractMatrix, errors::AbstractMatrix,
                      converged::AbstractVector{Bool})                                 # one device call
    @assert size(syndromes, 2) == size(errors, 2)
    @assert size(syndromes, 2) == length(converged)
    size(syndromes, 1) == d.s && size(errors, 1) == d.n || throw(DimensionMismatch("syndromes / errors rows"))
    B = size(syndromes, 2)
    B == 0 && return errors, converged
    direct = errors isa Matrix{UInt8} || errors isa Matrix{Bool}
    err = direct ? reinterpret(UInt8, errors) : Matrix{UInt8}(undef, d.n, B)
    conv = Vector{UInt8}(undef, B)
    relay_call(d.handle, B, bitflip_image(syndromes), err, conv, C_NULL)
    direct || (errors .= err)
    converged .= conv .!= 0
    d.err .= view(err, :, B)
    return errors, converged
end
batchdecode!(d::MI355XRelayDecoder, syndromes::AbstractMatrix, errors::AbstractMatrix) =
    batchdecode!(d, syndromes, errors, Vector{Bool}(undef, size(syndromes, 2)))

# ---------------------------------------------------------------------------------------------
# Monte-Carlo trials over ldpc_trials_* (host entries): what the reference's tests do around every decode
# (test/test_bp_decoder.jl:19-30) -- errors = rand(n, B) .< per, syndromes = H * errors .% 2, guesses[:, i] == errors[:, i]
# -- with the sampling, syndrome and score rules of include/ldpc_mi355x.h.  These symbols were added without a change of
# the ABI version; `Libdl.dlsym(Libdl.dlopen(libldpc), :ldpc_trials_create; throw_error=false)` tells whether they exist.
# ---------------------------------------------------------------------------------------------
mutable struct Trials
    s::Int; n::Int; nl::Int
    handle::Ptr{Cvoid}
end

"""
    Trials(H; logicals=nothing, device=-1, kernel_variant=0)

`logicals`: an nl x n matrix whose rows are checked against `guess .⊻ error` (flag bit 2 of `score!`).
"""
function Trials(H; logicals=nothing, device::Integer=-1, kernel_variant::Integer=0)
    s, n = size(H)
    sp = dropzeros(SparseMatrixCSC{Bool,Int}(sparse(H)))
    colptr = Int64.(sp.colptr .- 1); rowval = Int64.(rowvals(sp) .- 1)
    nl = 0; lcolptr = Int64[]; lrowval = Int64[]
    if logicals !== nothing && size(logicals, 1) > 0
        size(logicals, 2) == n || throw(DimensionMismatch("logicals must have as many columns as H"))
        lsp = dropzeros(SparseMatrixCSC{Bool,Int}(sparse(logicals)))
        nl = size(logicals, 1); lcolptr = Int64.(lsp.colptr .- 1); lrowval = Int64.(rowvals(lsp) .- 1)
    end
    opts = zeros(Int32, 16); opts[1] = Int32(device); opts[2] = Int32(kernel_variant)   # ldpc_trials_options (64 bytes)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ldpc_trials_create, libldpc), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                s, n, length(rowval), colptr, rowval, nl, length(lrowval), nl > 0 ? pointer(lcolptr) : C_NULL,
                nl > 0 && !isempty(lrowval) ? pointer(lrowval) : C_NULL, opts, h))
    t = Trials(s, n, nl, h[])
    finalizer(t) do x
        x.handle != C_NULL && ccall((:ldpc_trials_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        x.handle = C_NULL
    end
    return t
end

"""
    sample!(t, errors, syndromes, per; seed=0, column0=0)

Fills `errors` (n x B, `Matrix{UInt8}` or `Matrix{Bool}`) and `syndromes` (s x B) by the header's sampling rule; column
`i` of the call is trial number `column0 + i - 1`.
"""
function sample!(t::Trials, errors::Union{Matrix{UInt8},Matrix{Bool}}, syndromes::Union{Matrix{UInt8},Matrix{Bool}},
                 per::Float64; seed::Integer=0, column0::Integer=0)
    size(errors, 1) == t.n && size(syndromes, 1) == t.s || throw(DimensionMismatch("errors / syndromes rows"))
    @assert size(errors, 2) == size(syndromes, 2)
    check(ccall((:ldpc_trials_sample, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Int64, Float64, UInt64, Ptr{UInt8}, Ptr{UInt8}),
                t.handle, size(errors, 2), column0, per, UInt64(seed), errors, syndromes))
    return errors, syndromes
end

"""
    set_rates!(t, rates)

One rate per bit (`rates[j]` in [0, 1], length n) for `sample_rates!`; `nothing` clears them.  Synchronous, and ordered
after every earlier call on the handle.
"""
function set_rates!(t::Trials, rates::Union{Nothing,AbstractVector{<:Real}})
    if rates === nothing
        check(ccall((:ldpc_trials_set_rates, libldpc), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), t.handle, t.n, C_NULL))
        return t
    end
    length(rates) == t.n || throw(DimensionMismatch("one rate per bit"))
    check(ccall((:ldpc_trials_set_rates, libldpc), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), t.handle, t.n, Vector{Float64}(rates)))
    return t
end

"""
    sample_rates!(t, errors, syndromes; seed=0, column0=0)

`sample!` with bit `j` drawn at `rates[j]` (`set_rates!`): equal to `sample!` in every element where all rates are equal.
"""
function sample_rates!(t::Trials, errors::Union{Matrix{UInt8},Matrix{Bool}}, syndromes::Union{Matrix{UInt8},Matrix{Bool}};
                       seed::Integer=0, column0::Integer=0)
    size(errors, 1) == t.n && size(syndromes, 1) == t.s || throw(DimensionMismatch("errors / syndromes rows"))
    @assert size(errors, 2) == size(syndromes, 2)
    check(ccall((:ldpc_trials_sample_rates, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Int64, UInt64, Ptr{UInt8}, Ptr{UInt8}),
                t.handle, size(errors, 2), column0, UInt64(seed), errors, syndromes))
    return errors, syndromes
end

"""
    sample_rates_device!(t, batch, d_errors, d_syndromes; seed=0, column0=0, stream=C_NULL)

The same with DEVICE pointers (`d_syndromes` may be `C_NULL`), asynchronous on `stream`.
"""
function sample_rates_device!(t::Trials, batch::Integer, d_errors::Ptr{UInt8}, d_syndromes::Ptr{UInt8};
                              seed::Integer=0, column0::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    check(ccall((:ldpc_trials_sample_rates_device, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Int64, UInt64, Ptr{UInt8}, Ptr{UInt8}, Ptr{Cvoid}),
                t.handle, batch, column0, UInt64(seed), d_errors, d_syndromes, stream))
    return nothing
end

"""
    score!(t, guesses, errors, counts=zeros(Int64, 4)) -> (flags, counts)

`flags[i]`: bit 0 `guesses[:, i] != errors[:, i]`, bit 1 the guess does not reproduce the syndrome, bit 2 a logical row
is hit.  `counts` = (columns, block errors, syndrome mismatches, logical errors) is ADDED to.
"""
function score!(t::Trials, guesses::Union{Matrix{UInt8},Matrix{Bool}}, errors::Union{Matrix{UInt8},Matrix{Bool}},
                counts::Vector{Int64}=zeros(Int64, 4))
    size(guesses) == size(errors) && size(errors, 1) == t.n || throw(DimensionMismatch("guesses / errors"))
    length(counts) == 4 || throw(DimensionMismatch("counts must hold 4 entries"))
    flags = Vector{UInt8}(undef, size(errors, 2))
    check(ccall((:ldpc_trials_score, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int64}),
                t.handle, size(errors, 2), guesses, errors, flags, counts))
    return flags, counts
end

# ---------------------------------------------------------------------------------------------
# Monte-Carlo trials of a CSS code over ldpc_css_trials_* (host entries): Pauli errors (ex, ez) by one draw per qubit,
# sz = Hz * ex .% 2 and sx = Hx * ez .% 2, and the joint score with logical X / Z failures (include/ldpc_mi355x.h).
# Symbols added without a change of the ABI version, as those of Trials.
# ---------------------------------------------------------------------------------------------
struct CSSPattern            # ldpc_css_pattern
    rows::Int64; nnz::Int64
    colptr::Ptr{Int64}; rowval::Ptr{Int64}
end

mutable struct CSSTrials
    n::Int; rows_x::Int; rows_z::Int; nlx::Int; nlz::Int
    handle::Ptr{Cvoid}
end

"""
    CSSTrials(Hx, Hz; Lx=nothing, Lz=nothing, device=-1, kernel_variant=0)

`Lx`, `Lz`: logical rows (flag bits 3 and 2 of `score!`).  The library does not require `Hx * Hz' == 0`.
"""
function CSSTrials(Hx, Hz; Lx=nothing, Lz=nothing, device::Integer=-1, kernel_variant::Integer=0)
    n = size(Hx, 2)
    size(Hz, 2) == n || throw(DimensionMismatch("Hx and Hz must have the same number of columns"))
    mats = Any[Hx, Hz, Lx, Lz]
    keep = Any[]; pats = Vector{Any}(undef, 4)
    for (k, M) in enumerate(mats)
        if M === nothing || size(M, 1) == 0
            pats[k] = C_NULL
            continue
        end
        size(M, 2) == n || throw(DimensionMismatch("logicals must have as many columns as Hx and Hz"))
        sp = dropzeros(SparseMatrixCSC{Bool,Int}(sparse(M)))
        colptr = Int64.(sp.colptr .- 1); rowval = Int64.(rowvals(sp) .- 1)
        push!(keep, colptr, rowval)
        pats[k] = Ref(CSSPattern(size(M, 1), length(rowval), pointer(colptr), isempty(rowval) ? C_NULL : pointer(rowval)))
    end
    opts = zeros(Int32, 16); opts[1] = Int32(device); opts[2] = Int32(kernel_variant)   # ldpc_css_trials_options (64 bytes)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep pats begin
        check(ccall((:ldpc_css_trials_create, libldpc), Cint,
                    (Int64, Ptr{CSSPattern}, Ptr{CSSPattern}, Ptr{CSSPattern}, Ptr{CSSPattern}, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                    n, pats[1], pats[2], pats[3], pats[4], opts, h))
    end
    nrows(M) = M === nothing ? 0 : size(M, 1)
    t = CSSTrials(n, size(Hx, 1), size(Hz, 1), nrows(Lx), nrows(Lz), h[])
    finalizer(t) do x
        x.handle != C_NULL && ccall((:ldpc_css_trials_destroy, libldpc), Cint, (Ptr{Cvoid},), x.handle)
        x.handle = C_NULL
    end
    return t
end

"""
    sample!(t::CSSTrials, ex, ez, sx, sz, (px, py, pz); seed=0, column0=0)

Fills `ex`, `ez` (n x B) and the syndromes `sx` (rows of Hx x B), `sz` (rows of Hz x B) by the header's Pauli rule.
"""
function sample!(t::CSSTrials, ex::Matrix{UInt8}, ez::Matrix{UInt8}, sx::Matrix{UInt8}, sz::Matrix{UInt8},
                 p::NTuple{3,Float64}; seed::Integer=0, column0::Integer=0)
    size(ex) == size(ez) && size(ex, 1) == t.n || throw(DimensionMismatch("ex / ez"))
    size(sx, 1) == t.rows_x && size(sz, 1) == t.rows_z || throw(DimensionMismatch("sx / sz rows"))
    @assert size(sx, 2) == size(ex, 2) == size(sz, 2)
    check(ccall((:ldpc_css_trials_sample, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, UInt64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}),
                t.handle, size(ex, 2), column0, p[1], p[2], p[3], UInt64(seed), ex, ez, sx, sz))
    return ex, ez, sx, sz
end

"""
    score!(t::CSSTrials, gx, gz, ex, ez, counts=zeros(Int64, 6)) -> (flags, counts)

`flags[i]`: bit 0 a guess differs, bit 1 a syndrome is not reproduced, bit 2 a logical X failure, bit 3 a logical Z
failure.  `counts` = (columns, bit 0, bit 1, bit 2 or 3, bit 2, bit 3) is ADDED to.
"""
function score!(t::CSSTrials, gx::Matrix{UInt8}, gz::Matrix{UInt8}, ex::Matrix{UInt8}, ez::Matrix{UInt8},
                counts::Vector{Int64}=zeros(Int64, 6))
    size(gx) == size(gz) == size(ex) == size(ez) && size(ex, 1) == t.n || throw(DimensionMismatch("guesses / errors"))
    length(counts) == 6 || throw(DimensionMismatch("counts must hold 6 entries"))
    flags = Vector{UInt8}(undef, size(ex, 2))
    check(ccall((:ldpc_css_trials_score, libldpc), Cint,
                (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int64}),
                t.handle, size(ex, 2), gx, gz, ex, ez, flags, counts))
    return flags, counts
end

end # module
