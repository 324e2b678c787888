"""Guided-decimation min-sum decoder (belief propagation with guided decimation, BPGD: Yao, Abu Laban, Häger, Amat,
Pfister, 2023): normalised min-sum in rounds of `max_iters` iterations; a round that ends without a solution hard-fixes
the most reliable undecided bit, keeps the messages and goes on -- over the ldpc_decim_* entry points (the rule is stated
in include/ldpc_mi355x.h).  Not a decoder of the reference.  Its argument order and methods are those of `MinSumDecoder`,
so `run_trials`, `run_css_trials`, `run_dem_trials`, `SlidingWindowDecoder` and
`BeliefPropagationOSDDecoder(bp_decoder=...)` drive it unchanged.  The library computes no logarithm: the prior LLRs are
formed here with numpy, and `.channel_llr` is the array actually handed over."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _capi, _host
from ._host import (Handle, _pattern_of, as_int, channel_prior, csc_arrays, current_device, device_option, host_batch,
                    host_ptr, one_prior_given, refuse_zero_alpha_clip, stream_ptr, tensor_ptr)
from .decoder import AbstractDecoder
from .minsum import MinSumScratchSpace


class DecimatedMinSumDecoder(AbstractDecoder, Handle):
    """`DecimatedMinSumDecoder(H, per, max_iters)` with a uniform prior, or one of `channel_probs=` / `channel_llr=`
    instead of `per`: exactly one of the three.  `max_iters` is the iterations of a ROUND; after a round without a
    solution the undecided bit of largest |LLR| is fixed to its sign (it reads +-2 clip from then on), at most
    `max_decimations` times (None: n, every bit), so a syndrome runs at most `max_iters * (max_decimations + 1)`
    iterations.  With `max_decimations=0` this is `MinSumDecoder(H, per, max_iters)`.  alpha, clip, kernel_variant: as
    `MinSumDecoder` (`.kernel` tells which tier the handle takes)."""

    _destroy = "ldpc_decim_destroy"
    _scratch_keeps = ("err", "log_probabs")
    decode_, batchdecode_ = _host.decode_, _host.batchdecode_

    def __init__(self, H, per: Optional[float] = None, max_iters: int = 10, *, channel_probs=None, channel_llr=None,
                 max_decimations: Optional[int] = None, alpha: float = 0.75, clip: float = 1e6,
                 device: Optional[int] = None, kernel_variant: int = 0):
        max_iters = as_int(max_iters, "max_iters")
        one_prior_given(per, channel_probs, channel_llr)
        if max_iters < 0:
            raise ValueError("max_iters must be >= 0")
        M = _pattern_of(H)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        max_decimations = self.n if max_decimations is None else as_int(max_decimations, "max_decimations", " or None")
        if not 0 <= max_decimations <= self.n:
            raise ValueError(f"max_decimations must lie in 0 .. n = {self.n}")
        self.channel_llr = channel_prior(self.n, per, channel_probs, channel_llr)
        self.per = None if per is None else float(per)
        self.max_iters, self.max_decimations = max_iters, max_decimations
        self.alpha, self.clip = float(alpha), float(clip)
        refuse_zero_alpha_clip(self.alpha, self.clip)
        self.scratch = MinSumScratchSpace(self.n)
        self.device = current_device() if device is None else device   # (what info() answers)
        colptr, rowval = csc_arrays(M)
        opts = _capi.DecimOptions()
        opts.device = device_option(self.device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant = int(kernel_variant)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_decim_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.channel_llr.ctypes.data, max_iters, max_decimations, ctypes.byref(opts))

    @property
    def kernel(self) -> int:
        """1 = on-chip (state in LDS), 2 = unlimited (state in a global workspace) (ldpc_decim_kernel)."""
        return int(self._L.ldpc_decim_kernel(self._h))

    def info(self):
        """`.device`: the GPU the handle lives on; `.kernel`: its tier; `.tile_syndromes`: the syndromes a workgroup decodes
        at a time (S); `.last_grid`: the workgroups of the most recent launch (0 before any) -- fewer than ceil(batch / S)
        means that a workgroup took a further tile in the same LDS block or workspace slot."""
        return SimpleNamespace(device=self.device, kernel=self.kernel,
                               tile_syndromes=int(self._L.ldpc_decim_tile_syndromes(self._h)),
                               last_grid=int(self._L.ldpc_decim_last_grid(self._h)))

    def decode_batch_host(self, syn_bs, want_llr: bool = False, want_decimated: bool = False):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, llr [B][n] f64 | None, iters [B] i32), and with
        want_decimated a fifth entry: decimated [B] i32, the bits fixed when the syndrome stopped.  llr is the posterior
        as it stood then; a fixed bit reads +-2 clip."""
        syn, B, err, conv, llr, its = host_batch(syn_bs, self.s, self.n, want_llr)
        dec = np.empty(B, dtype=np.int32) if want_decimated else None
        _capi.check(self._L.ldpc_decim_decode_batch(self._h, B, syn.ctypes.data, err.ctypes.data, conv.ctypes.data,
                                                    host_ptr(llr), its.ctypes.data, host_ptr(dec)), self._L)
        return (err, conv, llr, its, dec) if want_decimated else (err, conv, llr, its)

    def decode_batch_device(self, syn, err, conv, llr=None, iters=None, decimated=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, syn [B][s] u8, err [B][n] u8, conv [B] u8,
        llr [B][n] f64 | None, iters [B] i32 | None, decimated [B] i32 | None, all contiguous.  Asynchronous on `stream`
        (a hipStream_t as int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        _capi.check(self._L.ldpc_decim_decode_batch_device(
            self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)),
            tensor_ptr(conv, torch.uint8, B), tensor_ptr(llr, torch.float64, (B, self.n), optional=True),
            tensor_ptr(iters, torch.int32, B, optional=True), tensor_ptr(decimated, torch.int32, B, optional=True),
            stream_ptr(stream, syn)), self._L)
