"""Bit-flip decoder: host mirror of `BitFlipDecoder` (src/decoders/iterative_bitflip.jl:47-68) over the
ldpc_bitflip_* entry points; decode!/batchdecode! as in :116-201.  The reference breaks ties among the bits with the
largest vote with `rand`; the library's tie rule (include/ldpc_mi355x.h) is a pure function of (seed, column number,
iteration), and this object numbers the columns it decodes."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _capi, _host
from ._host import Handle, _pattern_of, as_int, csc_arrays, device_option, host_batch, stream_ptr, tensor_ptr
from .decoder import AbstractDecoder

TIE_BREAKS = {"random": _capi.BF_TIE_RANDOM, "first": _capi.BF_TIE_FIRST, "last": _capi.BF_TIE_LAST}


class BitFlipScratchSpace:
    """`BitFlipScratchSpace` (:3-23) as far as a caller reads it: `err` (returned by alias from decode!, :156) and a
    `votes`-shaped array.  The accumulated votes themselves live on the device and are not shipped back."""

    def __init__(self, s: int, n: int):
        self.err = np.zeros(n, dtype=np.int64)
        self.votes = np.zeros(n, dtype=np.int64)
        self.syn = np.zeros(s, dtype=np.int64)
        self.error_checks = np.zeros(s, dtype=np.int64)


class BitFlipDecoder(AbstractDecoder, Handle):
    """`BitFlipDecoder(H, per::Float64, max_iters::Int)`.  tie_break: "random" (default; seeded, reproducible), "first"
    or "last" among the maximisers in ascending bit order.  kernel_variant forces a tier (0 = auto).  decode!/batchdecode!
    (:116-201) leave the last column's `err` in the scratch."""

    _destroy = "ldpc_bitflip_destroy"
    _scratch_keeps = ("err",)
    decode_, batchdecode_ = _host.decode_, _host.batchdecode_

    def __init__(self, H, per: float, max_iters: int, *, tie_break="random", seed: int = 0, device: Optional[int] = None,
                 kernel_variant: int = 0):
        if not isinstance(per, float):
            raise TypeError("per must be a Float64")
        as_int(max_iters, "max_iters")
        M = _pattern_of(H)   # stored zeros dropped: only `true` entries of H count (`sparse_H[i, j]`, :135)
        self.per, self.max_iters = float(per), int(max_iters)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        self.scratch = BitFlipScratchSpace(self.s, self.n)
        self.tie_break = TIE_BREAKS[tie_break] if isinstance(tie_break, str) else int(tie_break)
        self.seed = int(seed)
        self.columns_decoded = 0   # column0 of the next call: repeated calls draw fresh tie-breaks, a seed replays a session
        colptr, rowval = csc_arrays(M)
        opts = _capi.BitFlipOptions()
        opts.device = device_option(device)
        opts.tie_break = self.tie_break
        opts.seed = self.seed & ((1 << 64) - 1)
        opts.kernel_variant = int(kernel_variant)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_bitflip_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.per, self.max_iters, ctypes.byref(opts))

    @property
    def kernel(self) -> int:
        """1 / 2 = on-chip (one wave / one workgroup per syndrome), 3 = unlimited, 4 = unlimited with 64-bit votes
        (ldpc_bitflip_kernel)."""
        return int(self._L.ldpc_bitflip_kernel(self._h))

    def _column0(self, column0, batch: int) -> int:
        if column0 is not None:
            return int(column0)
        c = self.columns_decoded
        self.columns_decoded += batch
        return c

    def decode_batch_host(self, syn_bs, column0: Optional[int] = None):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, iters [B] i32, stop_reason [B] u8).  column0=None:
        the columns continue the numbering of this object (`columns_decoded`, advanced by B)."""
        syn, B, err, conv, _, its = host_batch(syn_bs, self.s, self.n)
        stop = np.empty(B, dtype=np.uint8)
        _capi.check(self._L.ldpc_bitflip_decode_batch(self._h, B, self._column0(column0, B), syn.ctypes.data, err.ctypes.data,
                                                      conv.ctypes.data, its.ctypes.data, stop.ctypes.data), self._L)
        return err, conv, its, stop

    def decode_batch_device(self, syn, err, conv, iters=None, stop_reason=None, stream: Optional[int] = None,
                            column0: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, syn [B][s] u8, err [B][n] u8, conv [B] u8,
        iters [B] i32 | None, stop_reason [B] u8 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as
        int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        args = (tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)), tensor_ptr(conv, torch.uint8, B),
                tensor_ptr(iters, torch.int32, B, optional=True), tensor_ptr(stop_reason, torch.uint8, B, optional=True),
                stream_ptr(stream, syn))
        _capi.check(self._L.ldpc_bitflip_decode_batch_device(self._h, B, self._column0(column0, B), *args), self._L)
