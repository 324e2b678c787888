"""Monte-Carlo trials on the device: the steps that surround every decode in the reference's own use
(test/test_bp_decoder.jl:19-30, benchmark/benchmarks.jl:8-11) -- `errors = rand(n, B) .< per`,
`syndromes = H * errors .% 2`, decode, `guesses[:, i] == errors[:, i]`, an error rate -- over the ldpc_trials_* entry
points, so that the batch never leaves the GPU.  The sampling, syndrome and score rules are stated in
include/ldpc_mi355x.h; `run_trials` loops sample -> a decoder's device entry -> score and reads back the four
counts and the number of unconverged columns.  A handle may hold one rate per bit (`set_rates`; `sample_rates` then
draws bit j at its own rate by the same rule): biased noise, the columns of a detector error model (dem.py)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi
from ._host import Handle, _pattern_of, csc_arrays, device_option, host_ptr, stream_ptr, tensor_ptr
from ._host import current_device as _current_device   # (importable from here as before)

_M64 = (1 << 64) - 1


class Trials(Handle):
    """Owns the Tanner graph of `H` and the optional `logicals` (nl x n) on a device.  kernel_variant: 0 = by size,
    1 = on-chip bit image, 2 = unlimited (`.kernel` tells which one the handle takes)."""

    _destroy = "ldpc_trials_destroy"

    def __init__(self, H, logicals=None, device: Optional[int] = None, kernel_variant: int = 0):
        M = _pattern_of(H)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        colptr, rowval = csc_arrays(M)
        self.nl = 0
        lcolptr = lrowval = None
        if logicals is not None:
            Lm = _pattern_of(logicals)
            if int(Lm.shape[1]) != self.n:
                raise AssertionError("logicals must have as many columns as H")
            self.nl = int(Lm.shape[0])
            if self.nl:
                lcolptr, lrowval = csc_arrays(Lm)
        if device is None:
            # the current device NOW is the handle's for good: what `_torch_device` answers later must not follow a
            # change of the current device between here and a `sample`
            device = _current_device()
        opts = _capi.TrialsOptions()
        opts.device = device_option(device)
        opts.kernel_variant = int(kernel_variant)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_trials_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, self.nl,
                     int(lrowval.size) if lrowval is not None else 0, host_ptr(lcolptr), host_ptr(lrowval), ctypes.byref(opts))
        self.device = device
        self.rates = None   # the array handed to set_rates, or None

    @property
    def kernel(self) -> int:
        """1 = on-chip bit image, 2 = unlimited (ldpc_trials_kernel)."""
        return int(self._L.ldpc_trials_kernel(self._h))

    def _torch_device(self):
        import torch

        return torch.device("cuda", int(self.device))

    # -- device forms (torch tensors, asynchronous on `stream`: a hipStream_t as int, default torch's current stream) --
    def _sample_out(self, B: int, out, stream):
        """The (errors, syndromes) tensors of a sample, and the last three arguments of its call: their addresses and the
        stream."""
        import torch

        if out is None:
            dev = self._torch_device()
            err = torch.empty((B, self.n), dtype=torch.uint8, device=dev)
            syn = torch.empty((B, self.s), dtype=torch.uint8, device=dev)
        else:
            err, syn = out
        return err, syn, (tensor_ptr(err, torch.uint8, (B, self.n)), tensor_ptr(syn, torch.uint8, (B, self.s), optional=True),
                          stream_ptr(stream, err))

    def sample(self, batch: int, per: float, seed: int = 0, column0: int = 0, out=None, stream: Optional[int] = None):
        """-> (errors [batch][n] u8, syndromes [batch][s] u8).  `out` = (errors, syndromes) to write into; a
        syndromes of None there skips them (errors only)."""
        B = int(batch)
        err, syn, args = self._sample_out(B, out, stream)
        _capi.check(self._L.ldpc_trials_sample_device(self._h, B, int(column0), float(per), int(seed) & _M64, *args), self._L)
        return err, syn

    def set_rates(self, rates) -> None:
        """One rate per bit (array-like of n floats in [0, 1]) for `sample_rates`; None clears them.  Synchronous, and
        ordered after every earlier call on the handle."""
        r = None
        if rates is not None:
            r = np.ascontiguousarray(rates, dtype=np.float64)
            if r.shape != (self.n,):
                raise ValueError(f"one rate per bit: expected {self.n} entries, got shape {r.shape}")
        _capi.check(self._L.ldpc_trials_set_rates(self._h, self.n, host_ptr(r)), self._L)
        self.rates = r

    def sample_rates(self, batch: int, seed: int = 0, column0: int = 0, out=None, stream: Optional[int] = None):
        """`sample` with bit j drawn at rates[j] (`set_rates`); equal to `sample` in every element where all rates are equal."""
        B = int(batch)
        err, syn, args = self._sample_out(B, out, stream)
        _capi.check(self._L.ldpc_trials_sample_rates_device(self._h, B, int(column0), int(seed) & _M64, *args), self._L)
        return err, syn

    def syndromes(self, errors, out=None, stream: Optional[int] = None):
        """errors [B][n] u8 -> syndromes [B][s] u8 (`H * errors .% 2`)."""
        import torch

        B = int(errors.shape[0])
        syn = torch.empty((B, self.s), dtype=torch.uint8, device=errors.device) if out is None else out
        _capi.check(self._L.ldpc_trials_syndromes_device(self._h, B, tensor_ptr(errors, torch.uint8, (B, self.n)),
                                                         tensor_ptr(syn, torch.uint8, (B, self.s)), stream_ptr(stream, errors)), self._L)
        return syn

    def score(self, guesses, errors, flags=None, counts=None, stream: Optional[int] = None, want_flags: bool = True):
        """guesses, errors [B][n] u8 -> (flags [B] u8, counts [4] i64).  `counts` is ACCUMULATED into (a fresh one
        starts at zero): trials, block errors, syndrome mismatches, logical errors.  want_flags=False: no flags."""
        import torch

        B = int(errors.shape[0])
        g, e = tensor_ptr(guesses, torch.uint8, (B, self.n)), tensor_ptr(errors, torch.uint8, (B, self.n))
        if flags is None and want_flags:
            flags = torch.empty(B, dtype=torch.uint8, device=errors.device)
        if counts is None:
            counts = torch.zeros(4, dtype=torch.int64, device=errors.device)
        _capi.check(self._L.ldpc_trials_score_device(self._h, B, g, e, tensor_ptr(flags, torch.uint8, B, optional=True),
                                                     tensor_ptr(counts, torch.int64, 4), stream_ptr(stream, errors)), self._L)
        return flags, counts

    # -- host forms (numpy, synchronous) ---------------------------------------------------------------------------
    def sample_host(self, batch: int, per: float, seed: int = 0, column0: int = 0):
        B = int(batch)
        err = np.empty((B, self.n), dtype=np.uint8)
        syn = np.empty((B, self.s), dtype=np.uint8)
        _capi.check(self._L.ldpc_trials_sample(self._h, B, int(column0), float(per), int(seed) & _M64, err.ctypes.data,
                                               syn.ctypes.data), self._L)
        return err, syn

    def sample_rates_host(self, batch: int, seed: int = 0, column0: int = 0):
        B = int(batch)
        err = np.empty((B, self.n), dtype=np.uint8)
        syn = np.empty((B, self.s), dtype=np.uint8)
        _capi.check(self._L.ldpc_trials_sample_rates(self._h, B, int(column0), int(seed) & _M64, err.ctypes.data, syn.ctypes.data),
                    self._L)
        return err, syn

    def score_host(self, guesses, errors, counts=None):
        """-> (flags [B] u8, counts [4] i64); `counts` (numpy int64[4]) is accumulated into."""
        g = np.ascontiguousarray(guesses, dtype=np.uint8)
        e = np.ascontiguousarray(errors, dtype=np.uint8)
        B = int(e.shape[0])
        assert g.shape == (B, self.n) and e.shape == (B, self.n)
        flags = np.empty(B, dtype=np.uint8)
        if counts is None:
            counts = np.zeros(4, dtype=np.int64)
        assert counts.dtype == np.int64 and counts.flags.c_contiguous and counts.size == 4
        _capi.check(self._L.ldpc_trials_score(self._h, B, g.ctypes.data, e.ctypes.data, flags.ctypes.data, counts.ctypes.data),
                    self._L)
        return flags, counts


@dataclass
class TrialResult:
    trials: int
    block_errors: int          # guess != error (the reference's count)
    syndrome_mismatches: int   # the guess does not reproduce the error's syndrome
    logical_errors: int        # L * (guess ^ error) != 0; 0 without logicals
    not_converged: int         # columns whose decoder flag was false

    @property
    def block_error_rate(self) -> float:
        return self.block_errors / self.trials if self.trials else 0.0

    @property
    def syndrome_mismatch_rate(self) -> float:
        return self.syndrome_mismatches / self.trials if self.trials else 0.0

    @property
    def logical_error_rate(self) -> float:
        return self.logical_errors / self.trials if self.trials else 0.0

    @property
    def not_converged_rate(self) -> float:
        return self.not_converged / self.trials if self.trials else 0.0


def _device_decode(decoder, syn, err, conv, first_trial: int):
    """One batch through the decoder's device entry; returns the error tensor that holds the guesses."""
    from .bitflip import BitFlipDecoder
    from .osd import BeliefPropagationOSDDecoder

    if isinstance(decoder, BeliefPropagationOSDDecoder):
        guesses, c, _ = decoder.batchdecode_device(syn)
        conv.copy_(c)
        return guesses
    if isinstance(decoder, BitFlipDecoder):
        decoder.decode_batch_device(syn, err, conv, column0=first_trial)
        return err
    decoder.decode_batch_device(syn, err, conv)   # BP, BP-OTS
    return err


def run_trials(decoder, trials: int, per=None, batch: int = 65536, seed: int = 0, logicals=None) -> TrialResult:
    """`trials` Monte-Carlo trials of `decoder` (BP, BP+OSD, BP-OTS or bit-flip) at physical error rate `per`
    (default: the decoder's): sample -> decode -> score in batches of `batch` (the last one ragged) on torch's current
    stream of the decoder's GPU; trial number c is column c of the sampling rule (and of the bit-flip tie rule), so the
    result does not depend on `batch`.  Only the four counts and the number of unconverged columns are read back.
    `per` may be an array-like of one rate per bit instead: the rates are set once and every batch is drawn with
    `sample_rates`."""
    import torch

    from .osd import BeliefPropagationOSDDecoder

    bp = decoder.bp_decoder if isinstance(decoder, BeliefPropagationOSDDecoder) else decoder
    rates = None
    if per is None:
        per = bp.per
    elif np.ndim(per) > 0:
        rates = np.ascontiguousarray(per, dtype=np.float64)
        if rates.shape != (int(bp.sparse_H.shape[1]),):
            raise ValueError(f"one rate per bit: expected {int(bp.sparse_H.shape[1])} entries, got shape {rates.shape}")
    device = bp.info().device if hasattr(bp, "info") else torch.cuda.current_device()
    dev = torch.device("cuda", int(device))
    total, batch = int(trials), int(batch)
    assert total >= 0 and batch > 0
    tr = Trials(bp.sparse_H, logicals, device=int(device))
    try:
        if rates is not None:
            tr.set_rates(rates)
        with torch.cuda.device(dev):
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            unconverged = torch.zeros((), dtype=torch.int64, device=dev)
            B = min(batch, max(total, 1))
            err = torch.empty((B, tr.n), dtype=torch.uint8, device=dev)
            syn = torch.empty((B, tr.s), dtype=torch.uint8, device=dev)
            guess = torch.empty((B, tr.n), dtype=torch.uint8, device=dev)
            conv = torch.empty(B, dtype=torch.uint8, device=dev)
            done = 0
            while done < total:
                b = min(B, total - done)
                e, sy, gu, cv = err[:b], syn[:b], guess[:b], conv[:b]
                if rates is None:
                    tr.sample(b, per, seed=seed, column0=done, out=(e, sy))
                else:
                    tr.sample_rates(b, seed=seed, column0=done, out=(e, sy))
                guesses = _device_decode(decoder, sy, gu, cv, done)
                tr.score(guesses, e, counts=counts, want_flags=False)
                unconverged += (cv == 0).sum()
                done += b
            c = counts.cpu().tolist()
            nc = int(unconverged.cpu())
    finally:
        tr.close()
    return TrialResult(trials=int(c[0]), block_errors=int(c[1]), syndrome_mismatches=int(c[2]), logical_errors=int(c[3]),
                       not_converged=nc)
