"""Joint X/Z (Pauli) min-sum decoder of a CSS code, over the ldpc_pauli_minsum_* entry points (the rule is stated in
include/ldpc_mi355x.h).  One decoder over both check matrices: every qubit carries three beliefs (X, Y, Z against I), so
the correlation a Y error puts between the two sides -- which two binary decoders throw away -- is used in both
directions.  Not a decoder of the reference.  The library computes no logarithm: the three prior tables are formed here
with numpy (float64 `log(P(I) / P(W))`, rounded once to float32) and `.prior_x`, `.prior_y`, `.prior_z` are the arrays
actually handed over."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _capi
from ._host import (Handle, _pattern_of, as_int, css_pattern, current_device, device_option, host_ptr, refuse_zero_alpha_clip,
                    stream_ptr, tensor_ptr)
from .css_trials import pauli_rates


def pauli_priors(probs) -> np.ndarray:
    """probs [n][3] = (px, py, pz) per qubit -> [3][n] float32: log((1 - px - py - pz) / pW) for W = X, Y, Z.  ValueError
    unless every pW > 0 and px + py + pz < 1."""
    q = np.asarray(probs, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError(f"one (px, py, pz) per qubit: expected shape (n, 3), got {q.shape}")
    rest = 1.0 - q[:, 0] - q[:, 1] - q[:, 2]
    if q.size and not (np.all(q > 0.0) and np.all(rest > 0.0)):   # (False for NaN as well)
        raise ValueError("every Pauli probability must be > 0 and px + py + pz < 1")
    return np.ascontiguousarray(np.log(rest[None, :] / q.T).astype(np.float32))


class PauliMinSumDecoder(Handle):
    """`PauliMinSumDecoder(Hx, Hz, p, max_iters)`: `p` as `pauli_rates` takes it (a float: depolarizing noise of total rate
    p; a triple (px, py, pz)), the same for every qubit -- or `p=None` and `pauli_probs=` an (n, 3) array of per-qubit
    (px, py, pz): exactly one of the two.  alpha in (0, 1] scales every check-to-qubit message, clip > 0 clamps the
    qubit-to-check values.  kernel_variant: 0 = by size, 1 = on-chip, 2 = unlimited (`.kernel` tells which tier the handle
    takes).  check: assert Hx * Hz' = 0 over GF(2), as `CSSTrials` does (the library does not).  Flooding schedule."""

    _destroy = "ldpc_pauli_minsum_destroy"

    def __init__(self, Hx, Hz, p=None, max_iters: int = 50, alpha: float = 0.75, clip: float = 1e6, pauli_probs=None,
                 kernel_variant: int = 0, device: Optional[int] = None, check: bool = True):
        as_int(max_iters, "max_iters")
        if (p is None) == (pauli_probs is None):
            raise TypeError("give exactly one of p and pauli_probs")
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
        self.max_iters, self.alpha, self.clip = int(max_iters), float(alpha), float(clip)
        refuse_zero_alpha_clip(self.alpha, self.clip)
        self.device = current_device() if device is None else device   # (what info() answers)
        pat_x, pat_z = css_pattern(Mx), css_pattern(Mz)
        opts = _capi.PauliMinSumOptions()
        opts.device = device_option(self.device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant = int(kernel_variant)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_pauli_minsum_create, self.n, ctypes.byref(pat_x), ctypes.byref(pat_z), self.prior_x.ctypes.data,
                     self.prior_y.ctypes.data, self.prior_z.ctypes.data, self.max_iters, ctypes.byref(opts))

    @property
    def kernel(self) -> int:
        """1 = on-chip (state in LDS), 2 = unlimited (state in a global workspace) (ldpc_pauli_minsum_kernel)."""
        return int(self._L.ldpc_pauli_minsum_kernel(self._h))

    @property
    def tile_syndromes(self) -> int:
        """The syndromes a workgroup decodes at a time (S)."""
        return int(self._L.ldpc_pauli_minsum_tile_syndromes(self._h))

    @property
    def last_grid(self) -> int:
        """The workgroups of the most recent launch (0 before any); fewer than ceil(batch / S): slots were reused."""
        return int(self._L.ldpc_pauli_minsum_last_grid(self._h))

    def info(self):
        return SimpleNamespace(device=self.device, kernel=self.kernel, tile_syndromes=self.tile_syndromes, last_grid=self.last_grid)

    def decode_batch_host(self, sx, sz, want_llr: bool = False):
        """sx [B][rows_x] (= Hx ez), sz [B][rows_z] (= Hz ex) uint8 -> (gx [B][n] u8, gz [B][n] u8, converged [B] u8,
        llr [B][3][n] f64 | None: the planes GX, GY, GZ, iters [B] i32)."""
        sx, sz = np.ascontiguousarray(sx, dtype=np.uint8), np.ascontiguousarray(sz, dtype=np.uint8)
        if sx.ndim != 2 or sz.ndim != 2 or sx.shape[1] != self.rows_x or sz.shape[1] != self.rows_z or sx.shape[0] != sz.shape[0]:
            raise AssertionError("syndrome shapes do not match the checks of Hx and Hz")
        B = int(sx.shape[0])
        gx, gz = np.empty((B, self.n), dtype=np.uint8), np.empty((B, self.n), dtype=np.uint8)
        conv = np.empty(B, dtype=np.uint8)
        llr = np.empty((B, 3, self.n), dtype=np.float64) if want_llr else None
        its = np.empty(B, dtype=np.int32)
        _capi.check(self._L.ldpc_pauli_minsum_decode_batch(self._h, B, sx.ctypes.data, sz.ctypes.data, gx.ctypes.data, gz.ctypes.data,
                                                           conv.ctypes.data, host_ptr(llr), its.ctypes.data), self._L)
        return gx, gz, conv, llr, its

    def decode_batch_device(self, sx, sz, gx, gz, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, sx [B][rows_x], sz [B][rows_z], gx, gz [B][n], conv [B]
        u8, llr [B][3][n] f64 | None, iters [B] i32 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as
        int; default = torch's current stream)."""
        import torch

        B = int(sx.shape[0])
        u8 = torch.uint8
        _capi.check(self._L.ldpc_pauli_minsum_decode_batch_device(
            self._h, B, tensor_ptr(sx, u8, (B, self.rows_x)), tensor_ptr(sz, u8, (B, self.rows_z)), tensor_ptr(gx, u8, (B, self.n)),
            tensor_ptr(gz, u8, (B, self.n)), tensor_ptr(conv, u8, B), tensor_ptr(llr, torch.float64, (B, 3, self.n), optional=True),
            tensor_ptr(iters, torch.int32, B, optional=True), stream_ptr(stream, sx)), self._L)
