"""Bit-flip decoder: host mirror of `BitFlipDecoder` (src/decoders/iterative_bitflip.jl:47-68) over the
ldpc_bitflip_* entry points; decode!/batchdecode! as in :116-201.  The reference breaks ties among the bits with the
largest vote with `rand`; the library's tie rule (include/ldpc_mi355x.h) is a pure function of (seed, column number,
iteration), and this object numbers the columns it decodes."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _capi
from .decoder import AbstractDecoder, _pattern_of, syndrome_bytes

TIE_BREAKS = {"random": _capi.BF_TIE_RANDOM, "first": _capi.BF_TIE_FIRST, "last": _capi.BF_TIE_LAST}


class BitFlipScratchSpace:
    """`BitFlipScratchSpace` (:3-23) as far as a caller reads it: `err` (returned by alias from decode!, :156) and a
    `votes`-shaped array.  The accumulated votes themselves live on the device and are not shipped back."""

    def __init__(self, s: int, n: int):
        self.err = np.zeros(n, dtype=np.int64)
        self.votes = np.zeros(n, dtype=np.int64)
        self.syn = np.zeros(s, dtype=np.int64)
        self.error_checks = np.zeros(s, dtype=np.int64)


class BitFlipDecoder(AbstractDecoder):
    """`BitFlipDecoder(H, per::Float64, max_iters::Int)`.  tie_break: "random" (default; seeded, reproducible), "first"
    or "last" among the maximisers in ascending bit order.  kernel_variant forces a tier (0 = auto)."""

    def __init__(self, H, per: float, max_iters: int, *, tie_break="random", seed: int = 0, device: Optional[int] = None,
                 kernel_variant: int = 0):
        if not isinstance(per, float):
            raise TypeError("per must be a Float64")
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)):
            raise TypeError("max_iters must be an Int")
        M = _pattern_of(H)   # stored zeros dropped: only `true` entries of H count (`sparse_H[i, j]`, :135)
        self.per, self.max_iters = float(per), int(max_iters)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        self.scratch = BitFlipScratchSpace(self.s, self.n)
        self.tie_break = TIE_BREAKS[tie_break] if isinstance(tie_break, str) else int(tie_break)
        self.seed = int(seed)
        self.columns_decoded = 0   # column0 of the next call: repeated calls draw fresh tie-breaks, a seed replays a session
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64)
        opts = _capi.BitFlipOptions()
        opts.device = -1 if device is None else int(device)
        opts.tie_break = self.tie_break
        opts.seed = self.seed & ((1 << 64) - 1)
        opts.kernel_variant = int(kernel_variant)
        self._h = ctypes.c_void_p()
        self._L = _capi.lib_for(None)
        _capi.check(self._L.ldpc_bitflip_create(self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                                                self.per, self.max_iters, ctypes.byref(opts), ctypes.byref(self._h)), self._L)

    @property
    def kernel(self) -> int:
        """1 / 2 = on-chip (one wave / one workgroup per syndrome), 3 = unlimited, 4 = unlimited with 64-bit votes
        (ldpc_bitflip_kernel)."""
        return int(self._L.ldpc_bitflip_kernel(self._h))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.ldpc_bitflip_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _column0(self, column0, batch: int) -> int:
        if column0 is not None:
            return int(column0)
        c = self.columns_decoded
        self.columns_decoded += batch
        return c

    def decode_batch_host(self, syn_bs, column0: Optional[int] = None):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, iters [B] i32, stop_reason [B] u8).  column0=None:
        the columns continue the numbering of this object (`columns_decoded`, advanced by B)."""
        syn = np.ascontiguousarray(syn_bs, dtype=np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.s:
            raise AssertionError("syndrome length does not match the number of checks")
        B = int(syn.shape[0])
        err = np.empty((B, self.n), dtype=np.uint8)
        conv = np.empty(B, dtype=np.uint8)
        its = np.empty(B, dtype=np.int32)
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
        for x in (syn, err, conv) + ((stop_reason,) if stop_reason is not None else ()):
            assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        assert tuple(syn.shape) == (B, self.s) and tuple(err.shape) == (B, self.n) and conv.numel() == B
        assert stop_reason is None or stop_reason.numel() == B
        if iters is not None:
            assert iters.is_cuda and iters.dtype == torch.int32 and iters.is_contiguous() and iters.numel() == B
        if stream is None:
            stream = torch.cuda.current_stream(syn.device).cuda_stream
        _capi.check(self._L.ldpc_bitflip_decode_batch_device(
            self._h, B, self._column0(column0, B), syn.data_ptr(), err.data_ptr(), conv.data_ptr(),
            iters.data_ptr() if iters is not None else None,
            stop_reason.data_ptr() if stop_reason is not None else None, ctypes.c_void_p(stream)), self._L)

    def decode_(self, syndrome) -> Tuple[np.ndarray, bool]:
        """`decode!(decoder::BitFlipDecoder, syndrome)`: (scratch.err as Int vector, converged)."""
        syn = syndrome_bytes(np.asarray(syndrome).reshape(-1))
        if syn.size != self.s:
            raise IndexError(f"syndrome has length {syn.size}, decoder has {self.s} checks")
        err, conv, _, _ = self.decode_batch_host(syn.reshape(1, -1))
        self.scratch.err[:] = err[0]
        return self.scratch.err, bool(conv[0])

    def batchdecode_(self, syndromes, errors, success=None):
        """`batchdecode!(decoder::BitFlipDecoder, syndromes, errors, converged)` (:189-201): one device call."""
        syndromes = np.asarray(syndromes)
        B = syndromes.shape[1]
        if success is None:
            success = np.empty(B, dtype=np.bool_)
        assert syndromes.shape[1] == errors.shape[1]                  # :190
        assert syndromes.shape[1] == len(success)                     # :191
        err, conv, _, _ = self.decode_batch_host(np.ascontiguousarray(syndrome_bytes(syndromes).T))
        errors[:, :] = err.T
        success[:] = conv.astype(np.bool_)
        if B > 0:
            self.scratch.err[:] = err[-1]
        return errors, success
