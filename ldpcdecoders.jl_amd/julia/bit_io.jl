# bit_io.jl -- marshalling of `batchdecode!`'s matrices without per-element loops; included by LDPCDecodersMI355X.jl and
# LDPCDecodersMI355XDropIn.jl (NOT EXECUTED in this repository's pipeline, like them).
#
# A `BitMatrix` (what the reference's test and doctest pass as `errors`: test/test_bp_decoder.jl:26,
# belief_propagation.jl:217) stores element (r, c) as bit (c-1)*rows + (r-1) of `chunks::Vector{UInt64}` -- exactly the
# layout of ldpc_bp_decode_batch_bits (include/ldpc_mi355x.h), which therefore reads / writes `chunks` in place with
# bit0 = 0.  `Matrix{UInt8}` / `Matrix{Bool}` are the byte entry's image already.  Anything else (the `Matrix{Int64}` of
# `(H * errors) .% 2`) is packed ONCE into a reusable BitVector of the staging object `st` (fields syn_bits, err_bits,
# syn_u8, err_u8, conv_u8).  The including module defines
#     bits_call(st, B, syn_words, syn_bit0, err_words, err_bit0, conv, llr)::Cint   # ldpc_bp_decode_batch[_multi]_bits
#     bytes_call(st, B, syn, err, conv, llr)::Cint                                  # ldpc_bp_decode_batch[_multi]
#     syndrome_byte(x)::UInt8
# The library was found to have the bits entries by symbol lookup (its ABI version did not change with them).

const ByteMatrix = Union{Matrix{UInt8},Matrix{Bool}}

has_bits_entry(lib) = Libdl.dlsym(Libdl.dlopen(lib), :ldpc_bp_decode_batch_bits; throw_error=false) !== nothing

# is every entry 0 or 1?  (an entry like 2 or 3 keeps its parity but can never be matched, :136 / :181: only the byte
# alphabet of the library can say that, so such a matrix takes the byte entry through `syndrome_byte`)
all_binary(A) = all(x -> (x == 0) | (x == 1), A)

"""
    marshal_batchdecode!(st, s, n, syndromes, errors, success)

One library call for `batchdecode!(decoder, syndromes, errors, success)` (belief_propagation.jl:220-231), choosing the
entry by the argument types; returns nothing, `errors` and `success` are filled.
"""
function marshal_batchdecode!(st, s::Int, n::Int, syndromes::AbstractMatrix, errors::AbstractMatrix,
                              success::AbstractVector{Bool}; llr=Ptr{Float64}(C_NULL))
    B = size(syndromes, 2)
    conv = success isa Vector{Bool} ? success : resize!(st.conv_u8, B)       # a Vector{Bool} is a byte per element
    syn_bytes = syndromes isa ByteMatrix
    err_bytes = errors isa ByteMatrix
    if syn_bytes && err_bytes
        # the byte entry on the caller's own arrays: no conversion loop at all
        GC.@preserve syndromes errors conv check(bytes_call(st, B, pointer(syndromes), pointer(errors), pointer(conv), llr))
    elseif !(syndromes isa BitMatrix) && !all_binary(syndromes)
        # exotic entries (2, 3, ... or exotic element types): the scalar fallback into the byte image
        resize!(st.syn_u8, s * B); resize!(st.err_u8, n * B)
        @inbounds for i in 1:B, r in 1:s
            st.syn_u8[(i - 1) * s + r] = syndrome_byte(syndromes[r, i])
        end
        GC.@preserve st conv check(bytes_call(st, B, pointer(st.syn_u8), pointer(st.err_u8), pointer(conv), llr))
        errors .= reshape(st.err_u8, n, B)                                   # 0/1 -> eltype(errors)  (:227)
    else
        # the bits entry: a BitMatrix goes in as it is, anything else is packed once (a chunked broadcast, no scalar loop)
        syn_chunks = if syndromes isa BitMatrix
            syndromes.chunks
        else
            resize!(st.syn_bits, s * B)
            st.syn_bits .= vec(syndromes) .!= 0
            st.syn_bits.chunks
        end
        err_chunks = errors isa BitMatrix ? errors.chunks : resize!(st.err_bits, n * B).chunks
        GC.@preserve syndromes errors st conv check(bits_call(st, B, pointer(syn_chunks), 0, pointer(err_chunks), 0, pointer(conv), llr))
        errors isa BitMatrix || (errors .= reshape(st.err_bits, n, B))       # :227
    end
    if !(success isa Vector{Bool})
        success .= st.conv_u8 .!= 0                                          # :226
    end
    return nothing
end

"""
    last_column!(st, s, n, syndromes, err_out, llr_out)

The reference's per-column loop (:224-228) leaves the scratch with the LAST column's decision and LLRs: that column is
decoded once more alone (deterministic per syndrome) with LLRs -- a batch of 1, through the byte entry.
"""
function last_column!(st, s::Int, n::Int, syndromes::AbstractMatrix, err_out::AbstractVector, llr_out::Vector{Float64})
    B = size(syndromes, 2)
    resize!(st.syn_u8, s); resize!(st.err_u8, n); resize!(st.conv_u8, 1)
    @inbounds for r in 1:s
        st.syn_u8[r] = syndrome_byte(syndromes[r, B])
    end
    GC.@preserve st llr_out check(bytes_call(st, 1, pointer(st.syn_u8), pointer(st.err_u8), pointer(st.conv_u8), pointer(llr_out)))
    err_out .= st.err_u8
    return nothing
end
