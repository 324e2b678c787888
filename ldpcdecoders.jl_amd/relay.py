"""Relay min-sum decoder: normalised min-sum with a per-bit memory strength gamma, run as a chain of legs (each leg with
another set of gamma, continuing from the posterior of the leg before), returning the lightest of the first `stop_after`
solutions -- over the ldpc_relay_* entry points (the rule is stated in include/ldpc_mi355x.h).  Not a decoder of the
reference.  Its argument order and methods are those of `MinSumDecoder`, so `run_trials`, `run_css_trials` and
`BeliefPropagationOSDDecoder(bp_decoder=...)` drive it unchanged.  The library draws no random number and computes no
logarithm: the prior LLRs and the gammas are formed here with numpy, and `.channel_llr`, `.gammas` and `.leg_iters` are
the arrays actually handed over."""
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


class RelayMinSumDecoder(AbstractDecoder, Handle):
    """`RelayMinSumDecoder(H, per, max_iters)` with a uniform prior, or one of `channel_probs=` / `channel_llr=` instead
    of `per`: exactly one of the three.  `legs` legs: leg 0 runs `max_iters` iterations, every later leg `leg_iters`.
    `gammas=` gives the [legs][n] memory strengths outright (each inside (-1, 1)); otherwise leg 0 is `gamma0` everywhere
    and legs 1... are drawn uniformly in `gamma_range` from `numpy.random.default_rng(seed)`.  A syndrome stops at its
    `stop_after`-th solution and the one of lowest prior weight is returned.  alpha, clip, kernel_variant: as
    `MinSumDecoder` (`.kernel` tells which tier the handle takes)."""

    _destroy = "ldpc_relay_destroy"
    _scratch_keeps = ("err", "log_probabs")
    decode_, batchdecode_ = _host.decode_, _host.batchdecode_

    def __init__(self, H, per: Optional[float] = None, max_iters: int = 30, *, channel_probs=None, channel_llr=None,
                 legs: int = 9, leg_iters: int = 20, gamma0: float = 0.125, gamma_range=(-0.24, 0.66), gammas=None,
                 seed: int = 0, stop_after: int = 1, alpha: float = 0.75, clip: float = 1e6,
                 device: Optional[int] = None, kernel_variant: int = 0):
        max_iters, leg_iters = as_int(max_iters, "max_iters"), as_int(leg_iters, "leg_iters")
        legs, stop_after = as_int(legs, "legs"), as_int(stop_after, "stop_after")
        one_prior_given(per, channel_probs, channel_llr)
        if legs < 1:
            raise ValueError("legs must be >= 1")
        if stop_after < 1:
            raise ValueError("stop_after must be >= 1")
        if max_iters < 0 or leg_iters < 0:
            raise ValueError("max_iters and leg_iters must be >= 0")
        M = _pattern_of(H)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        self.channel_llr = channel_prior(self.n, per, channel_probs, channel_llr)
        self.per = None if per is None else float(per)
        if gammas is not None:
            g = np.array(gammas, dtype=np.float32)
            if g.shape != (legs, self.n):
                raise ValueError(f"gammas must have shape ({legs}, {self.n}), got {g.shape}")
        else:
            lo, hi = float(gamma_range[0]), float(gamma_range[1])
            if not (-1.0 < lo <= hi < 1.0) or not -1.0 < float(gamma0) < 1.0:
                raise ValueError("gamma0 and gamma_range must lie inside (-1, 1), gamma_range ascending")
            g = np.empty((legs, self.n), dtype=np.float32)
            g[0] = np.float32(gamma0)
            g[1:] = np.random.default_rng(seed).uniform(lo, hi, size=(legs - 1, self.n)).astype(np.float32)
        self.gammas = np.ascontiguousarray(g, dtype=np.float32)
        self.leg_iters = np.ascontiguousarray([max_iters] + [leg_iters] * (legs - 1), dtype=np.int32)
        self.max_iters, self.legs, self.stop_after = max_iters, legs, stop_after
        self.alpha, self.clip = float(alpha), float(clip)
        refuse_zero_alpha_clip(self.alpha, self.clip)
        self.scratch = MinSumScratchSpace(self.n)
        self.device = current_device() if device is None else device   # (what info() answers)
        colptr, rowval = csc_arrays(M)
        opts = _capi.RelayOptions()
        opts.device = device_option(self.device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant, opts.stop_after = int(kernel_variant), stop_after
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_relay_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.channel_llr.ctypes.data, legs, self.gammas.ctypes.data, self.leg_iters.ctypes.data, ctypes.byref(opts))

    @property
    def kernel(self) -> int:
        """1 = on-chip (state in LDS), 2 = unlimited (state in a global workspace) (ldpc_relay_kernel)."""
        return int(self._L.ldpc_relay_kernel(self._h))

    def info(self):
        """`.device`: the GPU the handle lives on; `.kernel`: its tier; `.tile_syndromes`: the syndromes a workgroup decodes
        at a time (S); `.last_grid`: the workgroups of the most recent launch (0 before any) -- fewer than ceil(batch / S)
        means that a workgroup took a further tile in the same LDS block or workspace slot."""
        return SimpleNamespace(device=self.device, kernel=self.kernel,
                               tile_syndromes=int(self._L.ldpc_relay_tile_syndromes(self._h)),
                               last_grid=int(self._L.ldpc_relay_last_grid(self._h)))

    def decode_batch_host(self, syn_bs, want_llr: bool = False, want_solutions: bool = False):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, llr [B][n] f64 | None, iters [B] i32), and with
        want_solutions a fifth entry: solutions [B] i32.  llr is the posterior as it stood when the syndrome stopped."""
        syn, B, err, conv, llr, its = host_batch(syn_bs, self.s, self.n, want_llr)
        sol = np.empty(B, dtype=np.int32) if want_solutions else None
        _capi.check(self._L.ldpc_relay_decode_batch(self._h, B, syn.ctypes.data, err.ctypes.data, conv.ctypes.data,
                                                    host_ptr(llr), its.ctypes.data, host_ptr(sol)), self._L)
        return (err, conv, llr, its, sol) if want_solutions else (err, conv, llr, its)

    def decode_batch_device(self, syn, err, conv, llr=None, iters=None, solutions=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, syn [B][s] u8, err [B][n] u8, conv [B] u8,
        llr [B][n] f64 | None, iters [B] i32 | None, solutions [B] i32 | None, all contiguous.  Asynchronous on `stream`
        (a hipStream_t as int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        _capi.check(self._L.ldpc_relay_decode_batch_device(
            self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)),
            tensor_ptr(conv, torch.uint8, B), tensor_ptr(llr, torch.float64, (B, self.n), optional=True),
            tensor_ptr(iters, torch.int32, B, optional=True), tensor_ptr(solutions, torch.int32, B, optional=True),
            stream_ptr(stream, syn)), self._L)
