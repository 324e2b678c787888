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
from .css_trials import pauli_rates
from .decoder import _pattern_of
from .minsum import _current_device


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


class PauliMinSumDecoder:
    """`PauliMinSumDecoder(Hx, Hz, p, max_iters)`: `p` as `pauli_rates` takes it (a float: depolarizing noise of total rate
    p; a triple (px, py, pz)), the same for every qubit -- or `p=None` and `pauli_probs=` an (n, 3) array of per-qubit
    (px, py, pz): exactly one of the two.  alpha in (0, 1] scales every check-to-qubit message, clip > 0 clamps the
    qubit-to-check values.  kernel_variant: 0 = by size, 1 = on-chip, 2 = unlimited (`.kernel` tells which tier the handle
    takes).  check: assert Hx * Hz' = 0 over GF(2), as `CSSTrials` does (the library does not).  Flooding schedule."""

    def __init__(self, Hx, Hz, p=None, max_iters: int = 50, alpha: float = 0.75, clip: float = 1e6, pauli_probs=None,
                 kernel_variant: int = 0, device: Optional[int] = None, check: bool = True):
        self._h = None
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)):
            raise TypeError("max_iters must be an Int")
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
        if np.float32(self.alpha) == 0.0 or np.float32(self.clip) == 0.0:
            # a zero in ldpc_pauli_minsum_options selects the default there; here a default is spelled by leaving the
            # keyword out, so a zero gets the status the library gives every other value outside the range
            raise _capi.LdpcError(1, "alpha must lie in (0, 1] and clip must be finite and > 0 (got a zero)")
        if device is None:
            device = _current_device()   # the current device NOW is the handle's for good (what info() answers)
        self.device = device
        keep, pats = [], []
        for M in (Mx, Mz):
            colptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
            rowval = np.ascontiguousarray(M.indices, dtype=np.int64)
            keep += [colptr, rowval]
            pat = _capi.CSSPattern()
            pat.rows, pat.nnz, pat.colptr, pat.rowval = int(M.shape[0]), int(rowval.size), colptr.ctypes.data, rowval.ctypes.data
            pats.append(pat)
        opts = _capi.PauliMinSumOptions()
        opts.device = -1 if device is None else int(device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant = int(kernel_variant)
        h = ctypes.c_void_p()
        self._L = _capi.lib_for(None)
        _capi.check(self._L.ldpc_pauli_minsum_create(self.n, ctypes.byref(pats[0]), ctypes.byref(pats[1]), self.prior_x.ctypes.data,
                                                     self.prior_y.ctypes.data, self.prior_z.ctypes.data, self.max_iters,
                                                     ctypes.byref(opts), ctypes.byref(h)), self._L)
        self._h = h

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

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.ldpc_pauli_minsum_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
                                                           conv.ctypes.data, llr.ctypes.data if want_llr else None, its.ctypes.data),
                    self._L)
        return gx, gz, conv, llr, its

    def decode_batch_device(self, sx, sz, gx, gz, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, sx [B][rows_x], sz [B][rows_z], gx, gz [B][n], conv [B]
        u8, llr [B][3][n] f64 | None, iters [B] i32 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as
        int; default = torch's current stream)."""
        import torch

        B = int(sx.shape[0])
        for x in (sx, sz, gx, gz, conv):
            assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        assert tuple(sx.shape) == (B, self.rows_x) and tuple(sz.shape) == (B, self.rows_z)
        assert tuple(gx.shape) == (B, self.n) and tuple(gz.shape) == (B, self.n) and conv.numel() == B
        if llr is not None:
            assert llr.is_cuda and llr.dtype == torch.float64 and llr.is_contiguous() and tuple(llr.shape) == (B, 3, self.n)
        if iters is not None:
            assert iters.is_cuda and iters.dtype == torch.int32 and iters.is_contiguous() and iters.numel() == B
        if stream is None:
            stream = torch.cuda.current_stream(sx.device).cuda_stream
        _capi.check(self._L.ldpc_pauli_minsum_decode_batch_device(
            self._h, B, sx.data_ptr(), sz.data_ptr(), gx.data_ptr(), gz.data_ptr(), conv.data_ptr(),
            llr.data_ptr() if llr is not None else None, iters.data_ptr() if iters is not None else None, ctypes.c_void_p(stream)),
            self._L)
