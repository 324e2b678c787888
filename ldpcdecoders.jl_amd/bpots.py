"""BP-OTS decoder: host mirror of `BPOTSDecoder` (src/decoders/bpots_decoder.jl:39-115) over the
ldpc_bpots_* entry points; decode!/batchdecode! as in :225-340 and abstract_decoder.jl:31-48."""
from __future__ import annotations

from . import _capi, _host
from ._host import Handle, _pattern_of, csc_arrays, device_option, host_batch, stream_ptr, tensor_ptr
from .decoder import AbstractDecoder


class BPOTSDecoder(AbstractDecoder, Handle):
    """`BPOTSDecoder(H, per::Float64, max_iters::Int; T::Int=9, C::Float64=2.0)`.  `decode_` returns best_decisions as an
    Int vector; there is no host scratch."""

    _destroy = "ldpc_bpots_destroy"
    _scratch_keeps = ()
    decode_, batchdecode_ = _host.decode_, _host.batchdecode_

    def __init__(self, H, per: float, max_iters: int, *, T: int = 9, C: float = 2.0, device=None, experiments=None):
        if not isinstance(per, float):
            raise TypeError("per must be a Float64")
        M = _pattern_of(H)
        self.per, self.max_iters, self.T, self.C = float(per), int(max_iters), int(T), float(C)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        colptr, rowval = csc_arrays(M)
        L = _capi.lib_for(experiments)
        self._create(L, L.ldpc_bpots_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.per, self.max_iters, self.T, self.C, device_option(device))

    @property
    def kernel(self) -> int:
        """2 = LDS-resident kernel, 3 = node-parallel kernel with the messages in a global slot (ldpc_bpots_kernel)."""
        return int(self._L.ldpc_bpots_kernel(self._h))

    def decode_batch_host(self, syn_bs):
        """syn [B][s] uint8 -> (errors [B][n] u8 = best_decisions, converged [B] u8, iters [B] i32)."""
        syn, B, err, conv, _, its = host_batch(syn_bs, self.s, self.n)
        _capi.check(self._L.ldpc_bpots_decode_batch(self._h, B, syn.ctypes.data, err.ctypes.data,
                                                    conv.ctypes.data, its.ctypes.data), self._L)
        return err, conv, its

    def decode_batch_device(self, syn, err, conv, iters=None, stream=None) -> None:
        """HBM-resident batch (ldpc_bpots_decode_batch_device): torch tensors on the decoder's GPU, syn [B][s] u8,
        err [B][n] u8, conv [B] u8, iters [B] i32 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as
        int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        _capi.check(self._L.ldpc_bpots_decode_batch_device(
            self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)),
            tensor_ptr(conv, torch.uint8, B), tensor_ptr(iters, torch.int32, B, optional=True), stream_ptr(stream, syn)), self._L)
