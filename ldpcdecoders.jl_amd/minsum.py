"""Normalised min-sum decoder with one channel LLR per bit, over the ldpc_minsum_* entry points (the rule is stated in
include/ldpc_mi355x.h).  Not a decoder of the reference: it takes what the uniform `per` of the other decoders cannot
express -- biased noise, the two sides of a CSS code, soft input -- and its argument order matches
`BeliefPropagationDecoder`, so `run_trials`, `run_css_trials` and `BeliefPropagationOSDDecoder(bp_decoder=...)` drive it
unchanged.  The library computes no logarithm: the prior LLRs are formed here with numpy (float64 `log((1 - p) / p)`,
rounded once to float32) and `.channel_llr` is the array actually handed over."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _capi, _host
from ._host import (Handle, _pattern_of, as_int, channel_prior, csc_arrays, device_option, host_batch, host_ptr,
                    llr_of_probs, one_prior_given, refuse_zero_alpha_clip, stream_ptr, tensor_ptr)
from ._host import current_device as _current_device  # noqa: F401  (importable from here as before)
from .decoder import AbstractDecoder


class MinSumScratchSpace:
    """What a caller of the reference's decoders reads after a decode: `err` and `log_probabs` of the last column."""

    def __init__(self, n: int):
        self.err = np.zeros(n, dtype=np.float64)
        self.log_probabs = np.zeros(n, dtype=np.float64)


class MinSumDecoder(AbstractDecoder, Handle):
    """`MinSumDecoder(H, per, max_iters)` with a uniform prior, or one of `channel_probs=` (error probability per bit) /
    `channel_llr=` (log(P(0) / P(1)) per bit, finite) instead of `per`: exactly one of the three.  alpha in (0, 1]
    scales every check-to-bit message, clip > 0 clamps the bit-to-check values.  kernel_variant: 0 = by size, 1 = on-chip,
    2 = unlimited (`.kernel` tells which tier the handle takes).  schedule: "flooding" (every check reads the posteriors
    of the previous iteration) or "layered" (a check reads what the checks before it have just updated: THE LAYERED RULE
    of include/ldpc_mi355x.h; `.layers` tells the number of layers); anything else is a ValueError."""

    SCHEDULES = {"flooding": 0, "layered": 1}
    _destroy = "ldpc_minsum_destroy"
    _scratch_keeps = ("err", "log_probabs")
    decode_, batchdecode_ = _host.decode_, _host.batchdecode_

    def __init__(self, H, per: Optional[float] = None, max_iters: int = 50, *, channel_llr=None, channel_probs=None,
                 alpha: float = 0.75, clip: float = 1e6, device: Optional[int] = None, kernel_variant: int = 0,
                 schedule: str = "flooding"):
        if not isinstance(schedule, str) or schedule not in self.SCHEDULES:
            raise ValueError(f'schedule must be "flooding" or "layered", got {schedule!r}')
        self.schedule = schedule
        as_int(max_iters, "max_iters")
        one_prior_given(per, channel_probs, channel_llr)
        M = _pattern_of(H)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        self.channel_llr = channel_prior(self.n, per, channel_probs, channel_llr)
        self.per = None if per is None else float(per)
        self.max_iters, self.alpha, self.clip = int(max_iters), float(alpha), float(clip)
        refuse_zero_alpha_clip(self.alpha, self.clip)
        self.scratch = MinSumScratchSpace(self.n)
        self.conditional_llr = None   # (llr_if0, llr_if1) once set_conditional_priors has been called
        self.device = _current_device() if device is None else device   # (what info() answers)
        colptr, rowval = csc_arrays(M)
        opts = _capi.MinSumOptions()
        opts.device = device_option(self.device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant = int(kernel_variant)
        opts.schedule = self.SCHEDULES[schedule]
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_minsum_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.channel_llr.ctypes.data, self.max_iters, ctypes.byref(opts))

    @property
    def kernel(self) -> int:
        """1 = on-chip (state in LDS), 2 = unlimited (state in a global workspace) (ldpc_minsum_kernel)."""
        return int(self._L.ldpc_minsum_kernel(self._h))

    @property
    def layers(self) -> int:
        """The number of layers K of a layered handle; 0 for the flooding schedule (ldpc_minsum_layers)."""
        return int(self._L.ldpc_minsum_layers(self._h))

    def info(self):
        """`.device`: the GPU the handle lives on; `.kernel`: its tier; `.tile_syndromes`: the syndromes a workgroup decodes
        at a time (S); `.last_grid`: the workgroups of the most recent launch (0 before any) -- fewer than ceil(batch / S)
        means that a workgroup took a further tile in the same LDS block or workspace slot; `.schedule` and `.layers`:
        the schedule and its number of layers (0 for flooding); `.priors_kernel` and `.priors_tile_syndromes`: the tier
        and S of the entries with per-syndrome priors (the flooding schedule keeps a tile's priors beside its state, so
        they may differ from `.kernel` and `.tile_syndromes`; 0 where those entries are unsupported on the handle)."""
        return SimpleNamespace(device=self.device, kernel=self.kernel, schedule=self.schedule, layers=self.layers,
                               tile_syndromes=int(self._L.ldpc_minsum_tile_syndromes(self._h)),
                               last_grid=int(self._L.ldpc_minsum_last_grid(self._h)),
                               priors_kernel=int(self._L.ldpc_minsum_priors_kernel(self._h)),
                               priors_tile_syndromes=int(self._L.ldpc_minsum_priors_tile_syndromes(self._h)))

    def decode_batch_host(self, syn_bs, want_llr: bool = False):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, llr [B][n] f64 | None, iters [B] i32)."""
        syn, B, err, conv, llr, its = host_batch(syn_bs, self.s, self.n, want_llr)
        _capi.check(self._L.ldpc_minsum_decode_batch(self._h, B, syn.ctypes.data, err.ctypes.data, conv.ctypes.data,
                                                     host_ptr(llr), its.ctypes.data), self._L)
        return err, conv, llr, its

    def decode_batch_device(self, syn, err, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, syn [B][s] u8, err [B][n] u8, conv [B] u8,
        llr [B][n] f64 | None, iters [B] i32 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as int;
        default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        _capi.check(self._L.ldpc_minsum_decode_batch_device(
            self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)),
            tensor_ptr(conv, torch.uint8, B), tensor_ptr(llr, torch.float64, (B, self.n), optional=True),
            tensor_ptr(iters, torch.int32, B, optional=True), stream_ptr(stream, syn)), self._L)

    # -- per-syndrome priors (PER-SYNDROME PRIORS of include/ldpc_mi355x.h) ----------------------------------------------
    def _device_args(self, syn, extra, extra_dtype, err, conv, llr, iters, stream):
        """The arguments of a device entry that takes a [B][n] input `extra` next to the syndromes, after its checks."""
        import torch

        B = int(syn.shape[0])
        return (self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(extra, extra_dtype, (B, self.n)),
                tensor_ptr(err, torch.uint8, (B, self.n)), tensor_ptr(conv, torch.uint8, B),
                tensor_ptr(llr, torch.float64, (B, self.n), optional=True), tensor_ptr(iters, torch.int32, B, optional=True),
                stream_ptr(stream, syn))

    def decode_batch_priors_host(self, syn_bs, priors, want_llr: bool = False):
        """syn [B][s] uint8, priors [B][n] float32 (one prior LLR per syndrome and bit, in place of `.channel_llr`) ->
        (errors, converged, llr | None, iters) as `decode_batch_host`.  A row with a non-finite prior is not decoded:
        zeros, converged 0, iters 0, llr 0."""
        syn, B, err, conv, llr, its = host_batch(syn_bs, self.s, self.n, want_llr)
        pri = np.ascontiguousarray(priors, dtype=np.float32)
        if pri.shape != (B, self.n):
            raise ValueError(f"one prior per syndrome and bit: expected shape {(B, self.n)}, got {pri.shape}")
        _capi.check(self._L.ldpc_minsum_decode_batch_priors(self._h, B, syn.ctypes.data, pri.ctypes.data, err.ctypes.data, conv.ctypes.data,
                                                            host_ptr(llr), its.ctypes.data), self._L)
        return err, conv, llr, its

    def decode_batch_priors_device(self, syn, priors, err, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """`decode_batch_device` with priors [B][n] float32 on the decoder's GPU, contiguous."""
        import torch

        _capi.check(self._L.ldpc_minsum_decode_batch_priors_device(*self._device_args(syn, priors, torch.float32, err, conv, llr, iters, stream)),
                    self._L)

    def set_conditional_priors(self, llr_if0=None, llr_if1=None, *, probs_if0=None, probs_if1=None) -> None:
        """The two tables of the given-bits entries: the prior LLR of bit j where its given bit is 0 / 1.  Each as LLRs
        (finite, float32) or as error probabilities strictly inside (0, 1) (`probs_if0=` / `probs_if1=`, through
        `llr_of_probs`); a scalar stands for every bit.  May be called again: the next call decodes with the new tables.
        `.conditional_llr` holds the pair actually handed over."""
        tables = []
        for llr, probs, name in ((llr_if0, probs_if0, "if0"), (llr_if1, probs_if1, "if1")):
            if (llr is None) == (probs is None):
                raise TypeError(f"give exactly one of llr_{name} and probs_{name}")
            t = np.asarray(llr, dtype=np.float32) if llr is not None else llr_of_probs(probs)
            if t.ndim == 0:
                t = np.full(self.n, t, dtype=np.float32)
            if t.shape != (self.n,):
                raise ValueError(f"one entry per bit: expected {self.n} entries, got shape {t.shape}")
            tables.append(np.ascontiguousarray(t, dtype=np.float32))
        _capi.check(self._L.ldpc_minsum_set_conditional_priors(self._h, tables[0].ctypes.data, tables[1].ctypes.data), self._L)
        self.conditional_llr = (tables[0], tables[1])

    def decode_batch_given_host(self, syn_bs, given, want_llr: bool = False):
        """syn [B][s] uint8, given [B][n] uint8: the prior of bit j of row i is llr_if1[j] where given[i][j] & 1, else
        llr_if0[j] (`set_conditional_priors`) -> as `decode_batch_host`."""
        syn, B, err, conv, llr, its = host_batch(syn_bs, self.s, self.n, want_llr)
        giv = np.ascontiguousarray(given, dtype=np.uint8)
        if giv.shape != (B, self.n):
            raise ValueError(f"one given bit per syndrome and bit: expected shape {(B, self.n)}, got {giv.shape}")
        _capi.check(self._L.ldpc_minsum_decode_batch_given(self._h, B, syn.ctypes.data, giv.ctypes.data, err.ctypes.data, conv.ctypes.data,
                                                           host_ptr(llr), its.ctypes.data), self._L)
        return err, conv, llr, its

    def decode_batch_given_device(self, syn, given, err, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """`decode_batch_device` with given [B][n] uint8 on the decoder's GPU, contiguous."""
        import torch

        _capi.check(self._L.ldpc_minsum_decode_batch_given_device(*self._device_args(syn, given, torch.uint8, err, conv, llr, iters, stream)),
                    self._L)
