"""Pauli relay min-sum decoder of a CSS code, over the ldpc_pauli_relay_* entry points (the rule is stated in
include/ldpc_mi355x.h): the joint X/Z min-sum of `PauliMinSumDecoder` -- one decoder over both check matrices, three
beliefs a qubit -- run with the per-qubit memory strengths and the chain of legs of `RelayMinSumDecoder`, returning the
lightest of the first `stop_after` Pauli solutions.  Not a decoder of the reference.  Its first five positional arguments
and its device entry are those of `PauliMinSumDecoder`, so `run_css_joint_trials` drives it unchanged.  The library draws
no random number and computes no logarithm: the three prior tables and the gammas are formed here with numpy, exactly as
the two parents form them, and `.prior_x`, `.prior_y`, `.prior_z`, `.gammas` and `.leg_iters` are the arrays actually
handed over."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _capi
from ._host import (Handle, _pattern_of, as_int, css_pattern, current_device, device_option, host_ptr, refuse_zero_alpha_clip,
                    stream_ptr, tensor_ptr)
from .css_trials import pauli_rates
from .pauli import pauli_priors


class PauliRelayMinSumDecoder(Handle):
    """`PauliRelayMinSumDecoder(Hx, Hz, p, max_iters)`: `p` as `pauli_rates` takes it, the same for every qubit -- or
    `p=None` and `pauli_probs=` an (n, 3) array of per-qubit (px, py, pz): exactly one of the two, as `PauliMinSumDecoder`.
    `legs` legs: leg 0 runs `max_iters` iterations, every later leg `leg_iters`.  `gammas=` gives the [legs][n] memory
    strengths outright (each inside (-1, 1); one per qubit and leg, shared by its three beliefs); otherwise leg 0 is
    `gamma0` everywhere and legs 1... are drawn uniformly in `gamma_range` from `numpy.random.default_rng(seed)`, as
    `RelayMinSumDecoder` draws them.  A syndrome stops at its `stop_after`-th solution and the one of lowest prior weight
    is returned.  alpha, clip, kernel_variant, check: as `PauliMinSumDecoder` (`.kernel` tells which tier the handle
    takes)."""

    _destroy = "ldpc_pauli_relay_destroy"

    def __init__(self, Hx, Hz, p=None, max_iters: int = 30, *, pauli_probs=None, legs: int = 9, leg_iters: int = 20,
                 gamma0: float = 0.125, gamma_range=(-0.24, 0.66), gammas=None, seed: int = 0, stop_after: int = 1,
                 alpha: float = 0.75, clip: float = 1e6, kernel_variant: int = 0, device: Optional[int] = None, check: bool = True):
        max_iters, leg_iters = as_int(max_iters, "max_iters"), as_int(leg_iters, "leg_iters")
        legs, stop_after = as_int(legs, "legs"), as_int(stop_after, "stop_after")
        if (p is None) == (pauli_probs is None):
            raise TypeError("give exactly one of p and pauli_probs")
        if legs < 1:
            raise ValueError("legs must be >= 1")
        if stop_after < 1:
            raise ValueError("stop_after must be >= 1")
        if max_iters < 0 or leg_iters < 0:
            raise ValueError("max_iters and leg_iters must be >= 0")
        Mx, Mz = _pattern_of(Hx), _pattern_of(Hz)
        if int(Mx.shape[1]) != int(Mz.shape[1]):
            raise AssertionError("Hx and Hz must have the same number of columns")
        if check:
            prod = Mx.astype(np.int64) @ Mz.astype(np.int64).T
            if (prod.data % 2).any():
                raise AssertionError("Hx * Hz' != 0 over GF(2): the X and Z checks do not commute")
        self.sparse_Hx, self.sparse_Hz = Mx, Mz
        self.n, self.rows_x, self.rows_z = int(Mx.shape[1]), int(Mx.shape[0]), int(Mz.shape[0])
        if pauli_probs is None:
            pauli_probs = np.tile(np.array(pauli_rates(p), dtype=np.float64), (self.n, 1))
        priors = pauli_priors(pauli_probs)
        if priors.shape != (3, self.n):
            raise ValueError(f"one (px, py, pz) per qubit: expected {self.n} rows, got {priors.shape[1]}")
        self.prior_x, self.prior_y, self.prior_z = (np.ascontiguousarray(priors[k]) for k in range(3))
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
        self.device = current_device() if device is None else device   # (what info() answers)
        pat_x, pat_z = css_pattern(Mx), css_pattern(Mz)
        opts = _capi.PauliRelayOptions()
        opts.device = device_option(self.device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant, opts.stop_after = int(kernel_variant), stop_after
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_pauli_relay_create, self.n, ctypes.byref(pat_x), ctypes.byref(pat_z), self.prior_x.ctypes.data,
                     self.prior_y.ctypes.data, self.prior_z.ctypes.data, legs, self.gammas.ctypes.data, self.leg_iters.ctypes.data,
                     ctypes.byref(opts))

    @property
    def kernel(self) -> int:
        """1 = on-chip (state in LDS), 2 = unlimited (state in a global workspace) (ldpc_pauli_relay_kernel)."""
        return int(self._L.ldpc_pauli_relay_kernel(self._h))

    @property
    def tile_syndromes(self) -> int:
        """The syndromes a workgroup decodes at a time (S)."""
        return int(self._L.ldpc_pauli_relay_tile_syndromes(self._h))

    @property
    def last_grid(self) -> int:
        """The workgroups of the most recent launch (0 before any); fewer than ceil(batch / S): slots were reused."""
        return int(self._L.ldpc_pauli_relay_last_grid(self._h))

    def info(self):
        return SimpleNamespace(device=self.device, kernel=self.kernel, tile_syndromes=self.tile_syndromes, last_grid=self.last_grid)

    def decode_batch_host(self, sx, sz, want_llr: bool = False, want_solutions: bool = False):
        """sx [B][rows_x] (= Hx ez), sz [B][rows_z] (= Hz ex) uint8 -> (gx [B][n] u8, gz [B][n] u8, converged [B] u8,
        llr [B][3][n] f64 | None: the planes MX, MY, MZ as they stood when the syndrome stopped, iters [B] i32), and with
        want_solutions a sixth entry: solutions [B] i32."""
        sx, sz = np.ascontiguousarray(sx, dtype=np.uint8), np.ascontiguousarray(sz, dtype=np.uint8)
        if sx.ndim != 2 or sz.ndim != 2 or sx.shape[1] != self.rows_x or sz.shape[1] != self.rows_z or sx.shape[0] != sz.shape[0]:
            raise AssertionError("syndrome shapes do not match the checks of Hx and Hz")
        B = int(sx.shape[0])
        gx, gz = np.empty((B, self.n), dtype=np.uint8), np.empty((B, self.n), dtype=np.uint8)
        conv = np.empty(B, dtype=np.uint8)
        llr = np.empty((B, 3, self.n), dtype=np.float64) if want_llr else None
        its = np.empty(B, dtype=np.int32)
        sol = np.empty(B, dtype=np.int32) if want_solutions else None
        _capi.check(self._L.ldpc_pauli_relay_decode_batch(self._h, B, sx.ctypes.data, sz.ctypes.data, gx.ctypes.data, gz.ctypes.data,
                                                          conv.ctypes.data, host_ptr(llr), its.ctypes.data, host_ptr(sol)), self._L)
        return (gx, gz, conv, llr, its, sol) if want_solutions else (gx, gz, conv, llr, its)

    def decode_batch_device(self, sx, sz, gx, gz, conv, llr=None, iters=None, solutions=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, sx [B][rows_x], sz [B][rows_z], gx, gz [B][n], conv [B]
        u8, llr [B][3][n] f64 | None, iters [B] i32 | None, solutions [B] i32 | None, all contiguous.  Asynchronous on
        `stream` (a hipStream_t as int; default = torch's current stream)."""
        import torch

        B = int(sx.shape[0])
        u8 = torch.uint8
        _capi.check(self._L.ldpc_pauli_relay_decode_batch_device(
            self._h, B, tensor_ptr(sx, u8, (B, self.rows_x)), tensor_ptr(sz, u8, (B, self.rows_z)), tensor_ptr(gx, u8, (B, self.n)),
            tensor_ptr(gz, u8, (B, self.n)), tensor_ptr(conv, u8, B), tensor_ptr(llr, torch.float64, (B, 3, self.n), optional=True),
            tensor_ptr(iters, torch.int32, B, optional=True), tensor_ptr(solutions, torch.int32, B, optional=True),
            stream_ptr(stream, sx)), self._L)
