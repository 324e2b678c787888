"""Host-side mirror of the reference's decoder interface for the BP hot path.

Julia is not available in this image, so the host layer above the C ABI is
written in Python with the reference's names, argument meaning and error
behaviour (Julia's trailing ``!`` is spelled with a trailing underscore):

    BeliefPropagationDecoder(H, per, max_iters)   src/decoders/belief_propagation.jl:38-67
    reset_(decoder)            -> decoder          :83-91
    decode_(decoder, syndrome) -> (err, converged) :121-188
    batchdecode_(decoder, syndromes, errors[, success]) -> (errors, success)
                                                   :220-231, src/decoders/abstract_decoder.jl:31-48

All arithmetic happens in the HIP kernels behind ``libldpc_mi355x.so``; this
file only marshals arrays.  Matrices keep the reference's orientation:
``syndromes`` is ``s x B`` and ``errors`` is ``n x B`` (one column per sample).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from . import _capi
from ._host import Handle, _pattern_of, as_int, csc_arrays, device_option, host_syndromes, stream_ptr, syndrome_bytes, tensor_ptr
from .bitmatrix import BitMatrix


class AbstractDecoder:
    """`abstract type AbstractDecoder` (src/decoders/abstract_decoder.jl:9).

    A concrete decoder implements ``decode_(self, syndrome) -> (guess, converged)``.
    """

    def decode_(self, syndrome):  # pragma: no cover - interface
        raise NotImplementedError


class BeliefPropagationScratchSpace:
    """Host mirror of the fields other code reads (belief_propagation.jl:3-18):
    ``log_probabs`` (read by BP+OSD, belief_propagation_osd.jl:52) and ``err``
    (returned by alias from decode!, :187).  The message matrices themselves
    live in HBM in the layout described in DESIGN.md and are not exposed."""

    def __init__(self, n: int, s: int, per: float):
        self.log_probabs = np.zeros(n, dtype=np.float64)
        self.channel_probs = np.full(n, per, dtype=np.float64)
        self.err = np.zeros(n, dtype=np.float64)


class BeliefPropagationDecoder(AbstractDecoder, Handle):
    """Drop-in for `BeliefPropagationDecoder(H, per::Float64, max_iters::Int)`.

    Extra keyword arguments select the device and tuning knobs; defaults give
    the reference behaviour (``llr_exact=True``: LLRs from the full posterior odds instead of their upper 32 bits;
    include/ldpc_mi355x.h ldpc_bp_options).  ``devices=[0, 1, ...]`` makes ``batchdecode_`` / ``decode_batch_host`` /
    ``decode_batch_device`` partition the batch over those GPUs from this one process
    (ldpc_bp_create_multi: contiguous shards, one handle and stream per device; ``exchange`` picks how the
    root-device form moves shards: 0 auto, 1 hipMemcpyPeer, 2 RCCL).  ``experiments=True`` binds the build of
    the library that reads the environment knobs (default: only when one of them is set).
    """

    _destroy = "ldpc_bp_destroy"
    _m = None   # the multi-device handle when devices= is given

    def __init__(self, H, per: float, max_iters: int, *, device: Optional[int] = None,
                 devices: Optional[Sequence[int]] = None, exchange: int = 0,
                 waves_per_tile: int = 0, resident_tiles: int = 0, kernel_variant: int = 0,
                 defer_threshold: int = 0, llr_exact: bool = False, experiments: Optional[bool] = None):
        if not isinstance(per, float):
            raise TypeError("per must be a Float64 (reference signature: per::Float64)")
        as_int(max_iters, "max_iters", " (reference signature: max_iters::Int)")
        M = _pattern_of(H)
        self.per = float(per)
        self.max_iters = int(max_iters)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M                      # columns = bits      (:63)
        self.sparse_HT = sp.csc_matrix(M.T)    # columns = checks    (:64)
        self.sparse_HT.sort_indices()
        self.scratch = BeliefPropagationScratchSpace(self.n, self.s, self.per)
        colptr, rowval = csc_arrays(M)
        opts = _capi.BPOptions()
        opts.device = device_option(device)
        opts.waves_per_tile = int(waves_per_tile)
        opts.resident_tiles = int(resident_tiles)
        opts.kernel_variant = int(kernel_variant)   # 0 auto, 1 HBM-streaming, 2 LDS-resident, 3 node-parallel, 4 team
        opts.defer_threshold = int(defer_threshold)  # 0 auto (16), -1 off: straggler hand-off of the streaming kernel
        opts.llr_exact = 1 if llr_exact else 0       # LLRs from the full posterior odds (default: their upper 32 bits, within 5e-7)
        L = _capi.lib_for(experiments)
        graph = (self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, self.per, self.max_iters, ctypes.byref(opts))
        if devices is not None:
            if device is not None:
                raise TypeError("give device= or devices=, not both")
            devs = (ctypes.c_int32 * len(devices))(*[int(x) for x in devices])
            self._create(L, L.ldpc_bp_create_multi, len(devices), devs, int(exchange), *graph)
            self._m, self._h = self._h, ctypes.c_void_p(L.ldpc_bp_multi_handle(self._h, 0))   # info / timing: the root's handle
            self.devices = [int(x) for x in devices]
        else:
            self._create(L, L.ldpc_bp_create, *graph)
            self.devices = None

    def _check(self, status: int) -> None:
        _capi.check(status, self._L)

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        """With devices=, `_h` is the root's handle inside the multi-device one: destroying that one frees both."""
        m, self._m = self._m, None
        if m:
            self._h = None
            self._L.ldpc_bp_destroy_multi(m)
        else:
            super().close()

    # -- introspection ------------------------------------------------------
    def info(self) -> _capi.BPInfo:
        info = _capi.BPInfo()
        self._check(self._L.ldpc_bp_get_info(self._h, ctypes.byref(info)))
        return info

    def multi_info(self) -> _capi.BPMultiInfo:
        """devices, exchange kind and the scatter / decode / gather times of the most recent root-device call
        (ldpc_bp_multi_get_info); only with devices=."""
        assert self._m, "not a multi-device decoder"
        info = _capi.BPMultiInfo()
        self._check(self._L.ldpc_bp_multi_get_info(self._m, ctypes.byref(info)))
        return info

    def last_status(self) -> None:
        """Wait for everything enqueued on the handle and raise LdpcError if a team of workgroups lost a
        member in one of those calls (ldpc_bp_last_status): their outputs must then be decoded again."""
        if self._m:
            self._check(self._L.ldpc_bp_multi_last_status(self._m))
        else:
            self._check(self._L.ldpc_bp_last_status(self._h))

    def last_timing(self, calls_back: int = 0) -> Tuple[float, float, int]:
        """(sweep_ms, total_ms, sum_iters) of a recent batch call (0 = the latest), from HIP
        events recorded on the stream the kernels ran on."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        self._check(self._L.ldpc_bp_call_timing(self._h, calls_back, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def phase_ticks(self, calls_back: int = 0) -> Tuple[int, int, int]:
        """Diagnostics: 100 MHz ticks in (check sweep, variable sweep, convergence test), summed over workgroups."""
        t = (ctypes.c_uint64 * 3)()
        self._check(self._L.ldpc_bp_call_phase_ticks(self._h, calls_back, ctypes.byref(t)))
        return int(t[0]), int(t[1]), int(t[2])

    # -- raw ABI calls ------------------------------------------------------
    def decode_batch_host(self, syn_bs: np.ndarray, want_llr: bool = False, want_iters: bool = False, out=None):
        """syn_bs: [B][s] uint8 C-contiguous.  Returns (errors [B][n] u8, converged [B] u8, llr|None, iters|None).
        `out` = (errors, converged) preallocated C-contiguous uint8 arrays to write into (a caller that
        reuses its buffers, like Julia's batchdecode!, avoids fresh-page faults on every call)."""
        syn_bs = host_syndromes(syn_bs, self.s)
        B = int(syn_bs.shape[0])
        if out is not None:
            err, conv = out
            assert err.dtype == np.uint8 and err.flags.c_contiguous and err.shape == (B, self.n)
            assert conv.dtype == np.uint8 and conv.flags.c_contiguous and conv.shape == (B,)
        else:
            err = np.empty((B, self.n), dtype=np.uint8)   # every byte is written by the library
            conv = np.empty(B, dtype=np.uint8)
        llr = np.empty((B, self.n), dtype=np.float64) if want_llr else None
        its = np.empty(B, dtype=np.int32) if want_iters else None
        entry, handle = (self._L.ldpc_bp_decode_batch_multi, self._m) if self._m else (self._L.ldpc_bp_decode_batch, self._h)
        self._check(entry(handle, B, syn_bs.ctypes.data, err.ctypes.data, conv.ctypes.data,
                          llr.ctypes.data if want_llr else None, its.ctypes.data if want_iters else None))
        return err, conv, llr, its

    def decode_batch_device(self, syn, err, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch CUDA(HIP) tensors, syn [B][s] u8, err [B][n] u8, conv [B] u8,
        llr [B][n] f64 | None, iters [B] i32 | None, all contiguous.  Asynchronous on `stream`
        (a hipStream_t as int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        entry, handle = ((self._L.ldpc_bp_decode_batch_multi_device, self._m) if self._m
                         else (self._L.ldpc_bp_decode_batch_device, self._h))   # multi: the tensors live on devices[0]
        self._check(entry(handle, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)),
                          tensor_ptr(conv, torch.uint8, B), tensor_ptr(llr, torch.float64, (B, self.n), optional=True),
                          tensor_ptr(iters, torch.int32, B, optional=True), stream_ptr(stream, syn)))

    # -- bit-packed (BitMatrix layout) entries --------------------------------
    def decode_batch_bits_words(self, batch: int, syn_words: np.ndarray, syn_bit0: int, err_words: np.ndarray,
                                err_bit0: int, want_llr: bool = False, want_iters: bool = False):
        """ldpc_bp_decode_batch_bits (ldpc_bp_decode_batch_multi_bits with devices=) on host word vectors: the syndrome
        bit of (check r, column i) is bit syn_bit0 + i*s + r of `syn_words`, the error bit of (bit j, column i) becomes
        bit err_bit0 + i*n + j of `err_words` (uint64, written in place; no other bit changes).
        Returns (converged [B] u8, llr [B][n] | None, iters [B] | None)."""
        B = int(batch)
        for w, bit0, r in ((syn_words, syn_bit0, self.s), (err_words, err_bit0, self.n)):
            if not (isinstance(w, np.ndarray) and w.dtype == np.uint64 and w.ndim == 1 and w.flags.c_contiguous):
                raise TypeError("word vectors must be contiguous one-dimensional uint64 arrays")
            if B >= 0 and bit0 >= 0 and int(bit0) + B * r > 64 * w.size:
                raise IndexError("the bit range ends behind the word vector")   # BoundsError
        conv = np.empty(max(B, 0), dtype=np.uint8)
        llr = np.empty((B, self.n), dtype=np.float64) if want_llr else None
        its = np.empty(B, dtype=np.int32) if want_iters else None
        entry, handle = ((self._L.ldpc_bp_decode_batch_multi_bits, self._m) if self._m
                         else (self._L.ldpc_bp_decode_batch_bits, self._h))
        self._check(entry(handle, B, syn_words.ctypes.data, int(syn_bit0), err_words.ctypes.data, int(err_bit0),
                          conv.ctypes.data, llr.ctypes.data if want_llr else None, its.ctypes.data if want_iters else None))
        return conv, llr, its

    def decode_batch_bits_host(self, syn: BitMatrix, out: Optional[BitMatrix] = None, want_llr: bool = False,
                               want_iters: bool = False):
        """syn: BitMatrix s x B.  Returns (errors BitMatrix n x B, converged [B] u8, llr [B][n] | None, iters | None);
        `out` = a BitMatrix n x B to write into (every element is overwritten, its trailing bits stay as they are)."""
        if not isinstance(syn, BitMatrix):
            raise TypeError("syn must be a BitMatrix")
        if syn.rows != self.s:
            raise AssertionError("syndrome length does not match the number of checks")
        B = syn.cols
        if out is None:
            out = BitMatrix.zeros(self.n, B)
        elif not isinstance(out, BitMatrix) or out.shape != (self.n, B):
            raise AssertionError("out must be a BitMatrix of n x B")
        conv, llr, its = self.decode_batch_bits_words(B, syn.chunks, 0, out.chunks, 0, want_llr, want_iters)
        return out, conv, llr, its

    def decode_batch_bits_device(self, batch: int, syn_words, syn_bit0: int, err_words, err_bit0: int, conv,
                                 llr=None, iters=None, stream: Optional[int] = None) -> None:
        """HBM-resident bit strings: `syn_words` / `err_words` are contiguous one-dimensional torch tensors of 64-bit
        words (int64, or uint64 viewed as such) on the decoder's GPU, bit numbering as in decode_batch_bits_words;
        conv [B] u8, llr [B][n] f64 | None, iters [B] i32 | None.  Asynchronous on `stream` (ldpc_bp_decode_batch_bits_device)."""
        import torch

        if self._m:
            raise _capi.LdpcError(5, "decode_batch_bits_device: there is no root-device form of the bits entry "
                                     "(shard borders fall inside words; use decode_batch_bits_host with devices=, "
                                     "or a single-device decoder)")
        B = int(batch)
        for w in (syn_words, err_words):
            assert w.is_cuda and w.dim() == 1 and w.is_contiguous() and w.element_size() == 8 and not w.dtype.is_floating_point
        assert syn_bit0 >= 0 and int(syn_bit0) + B * self.s <= 64 * syn_words.numel()
        assert err_bit0 >= 0 and int(err_bit0) + B * self.n <= 64 * err_words.numel()
        self._check(self._L.ldpc_bp_decode_batch_bits_device(
            self._h, B, syn_words.data_ptr(), int(syn_bit0), err_words.data_ptr(), int(err_bit0), tensor_ptr(conv, torch.uint8, B),
            tensor_ptr(llr, torch.float64, (B, self.n), optional=True), tensor_ptr(iters, torch.int32, B, optional=True),
            stream_ptr(stream, conv)))

    # -- reference interface (methods; free functions below) ----------------
    def decode_(self, syndrome):
        return decode_(self, syndrome)


def reset_(decoder: BeliefPropagationDecoder) -> BeliefPropagationDecoder:
    """`reset!(bp_decoder)` (belief_propagation.jl:83-91).  Device scratch is reset
    inside every decode call, so only the host mirrors need clearing."""
    sc = decoder.scratch
    sc.log_probabs[:] = 0.0
    sc.channel_probs[:] = decoder.per
    sc.err[:] = 0.0
    return decoder


def decode_(decoder: BeliefPropagationDecoder, syndrome) -> Tuple[np.ndarray, bool]:
    """`decode!(decoder, syndrome)` (belief_propagation.jl:121-188).

    Returns ``(decoder.scratch.err, converged)``; like the reference the first
    element is the scratch vector itself (Float64 0.0/1.0), overwritten by the
    next call (:187)."""
    syn = syndrome_bytes(np.asarray(syndrome).reshape(-1))
    if syn.size != decoder.s:
        raise IndexError(f"syndrome has length {syn.size}, decoder has {decoder.s} checks")  # BoundsError
    reset_(decoder)
    err, conv, llr, _ = decoder.decode_batch_host(syn.reshape(1, -1), want_llr=True)
    decoder.scratch.err[:] = err[0]
    decoder.scratch.log_probabs[:] = llr[0]
    return decoder.scratch.err, bool(conv[0])


def batchdecode_(decoder: AbstractDecoder, syndromes, errors, success=None):
    """`batchdecode!(decoder, syndromes, errors[, success])`.

    For a BeliefPropagationDecoder the whole batch is one device call
    (belief_propagation.jl:220-231); any other AbstractDecoder takes the generic
    per-column loop (abstract_decoder.jl:31-42).  ``syndromes`` is ``s x B``,
    ``errors`` is ``n x B`` and is overwritten; ``success`` (length B, bool) is
    allocated when omitted (abstract_decoder.jl:44-48).  Returns
    ``(errors, success)``."""
    if isinstance(syndromes, BitMatrix) or isinstance(errors, BitMatrix):
        return _batchdecode_bits(decoder, syndromes, errors, success)
    syndromes = np.asarray(syndromes) if not isinstance(syndromes, np.ndarray) else syndromes
    if syndromes.ndim != 2 or errors.ndim != 2:
        raise TypeError("syndromes and errors must be matrices")
    B = syndromes.shape[1]
    if success is None:
        success = np.empty(B, dtype=np.bool_)                     # Vector{Bool}(undef, B)
    assert syndromes.shape[1] == errors.shape[1]                  # :221
    assert syndromes.shape[1] == len(success)                     # :222
    if hasattr(decoder, "batchdecode_") and not isinstance(decoder, BeliefPropagationDecoder):
        return decoder.batchdecode_(syndromes, errors, success)   # a decoder with its own batch strategy
    if not isinstance(decoder, BeliefPropagationDecoder):
        for i in range(B):                                        # abstract_decoder.jl:35-39
            guess, conv = decoder.decode_(syndromes[:, i])
            success[i] = conv
            errors[:, i] = guess
        return errors, success
    if syndromes.shape[0] != decoder.s or errors.shape[0] != decoder.n:
        raise IndexError("syndromes/errors row count does not match the decoder")
    syn_bs = syndrome_bytes(syndromes).T                          # [B][s]; a view for column-major input
    err, conv, _, _ = decoder.decode_batch_host(syn_bs)
    errors[:, :] = err.T                                          # 0/1 -> eltype(errors)  (:227)
    success[:] = conv.astype(np.bool_)                            # :226
    if B > 0:
        # the reference leaves the scratch holding the last column's result; the LLRs of
        # the whole batch are not shipped back for that, the last column is re-decoded alone
        _, _, llr, _ = decoder.decode_batch_host(syn_bs[-1:], want_llr=True)
        decoder.scratch.err[:] = err[-1]
        decoder.scratch.log_probabs[:] = llr[0]
    return errors, success


def _batchdecode_bits(decoder, syndromes, errors, success):
    """batchdecode_ when `syndromes` and / or `errors` is a BitMatrix: that argument goes to the bits entry as it is
    (no dense copy of it is made).  A dense `syndromes` next to a BitMatrix `errors` -- the shape of the reference's
    doctest -- is packed once."""
    if not isinstance(syndromes, BitMatrix):
        syndromes = np.asarray(syndromes)
    if syndromes.ndim != 2 or errors.ndim != 2:
        raise TypeError("syndromes and errors must be matrices")
    B = syndromes.shape[1]
    if success is None:
        success = np.empty(B, dtype=np.bool_)
    assert syndromes.shape[1] == errors.shape[1]                  # :221
    assert syndromes.shape[1] == len(success)                     # :222
    if not isinstance(decoder, BeliefPropagationDecoder):
        # the generic per-column loop (abstract_decoder.jl:31-42) works on dense columns
        dense_syn = syndromes.to_dense() if isinstance(syndromes, BitMatrix) else syndromes
        dense_err = np.zeros(errors.shape, dtype=np.uint8) if isinstance(errors, BitMatrix) else errors
        _, success = batchdecode_(decoder, dense_syn, dense_err, success)
        if isinstance(errors, BitMatrix):
            errors.chunks[:] = BitMatrix.from_dense(dense_err).chunks
        return errors, success
    if syndromes.shape[0] != decoder.s or errors.shape[0] != decoder.n:
        raise IndexError("syndromes/errors row count does not match the decoder")
    if not isinstance(syndromes, BitMatrix):
        syn_u8 = syndrome_bytes(syndromes)
        if syn_u8.size and syn_u8.max() > 1:
            # entries other than 0/1 (never matched, :181) have no bit form: the byte entry decodes, the result is packed
            dense_err = np.zeros(errors.shape, dtype=np.uint8)
            _, success = batchdecode_(decoder, syndromes, dense_err, success)
            errors.chunks[:] = BitMatrix.from_dense(dense_err).chunks
            return errors, success
        syndromes = BitMatrix.from_dense(syn_u8)                  # np.packbits, once
    out = errors if isinstance(errors, BitMatrix) else BitMatrix.zeros(decoder.n, B)
    _, conv, _, _ = decoder.decode_batch_bits_host(syndromes, out=out)
    if out is not errors:
        errors[:, :] = out.to_dense()                             # 0/1 -> eltype(errors)  (:227)
    success[:] = conv.astype(np.bool_)                            # :226
    if B > 0:
        # the scratch holds the last column's result, as after the reference's loop: that column is decoded alone
        last = BitMatrix.zeros(decoder.n, 1)
        _, llr, _ = decoder.decode_batch_bits_words(1, syndromes.chunks, (B - 1) * decoder.s, last.chunks, 0, want_llr=True)
        decoder.scratch.err[:] = last.column(0)
        decoder.scratch.log_probabs[:] = llr[0]
    return errors, success
