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
from typing import Optional, Tuple

import numpy as np

from . import _capi
from .decoder import AbstractDecoder, _pattern_of, syndrome_bytes
from .minsum import MinSumScratchSpace, _current_device, llr_of_probs


def _int(x, name: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{name} must be an Int")
    return int(x)


class RelayMinSumDecoder(AbstractDecoder):
    """`RelayMinSumDecoder(H, per, max_iters)` with a uniform prior, or one of `channel_probs=` / `channel_llr=` instead
    of `per`: exactly one of the three.  `legs` legs: leg 0 runs `max_iters` iterations, every later leg `leg_iters`.
    `gammas=` gives the [legs][n] memory strengths outright (each inside (-1, 1)); otherwise leg 0 is `gamma0` everywhere
    and legs 1... are drawn uniformly in `gamma_range` from `numpy.random.default_rng(seed)`.  A syndrome stops at its
    `stop_after`-th solution and the one of lowest prior weight is returned.  alpha, clip, kernel_variant: as
    `MinSumDecoder` (`.kernel` tells which tier the handle takes)."""

    def __init__(self, H, per: Optional[float] = None, max_iters: int = 30, *, channel_probs=None, channel_llr=None,
                 legs: int = 9, leg_iters: int = 20, gamma0: float = 0.125, gamma_range=(-0.24, 0.66), gammas=None,
                 seed: int = 0, stop_after: int = 1, alpha: float = 0.75, clip: float = 1e6,
                 device: Optional[int] = None, kernel_variant: int = 0):
        max_iters, leg_iters = _int(max_iters, "max_iters"), _int(leg_iters, "leg_iters")
        legs, stop_after = _int(legs, "legs"), _int(stop_after, "stop_after")
        if (per is not None) + (channel_llr is not None) + (channel_probs is not None) != 1:
            raise TypeError("give exactly one of per, channel_probs and channel_llr")
        if legs < 1:
            raise ValueError("legs must be >= 1")
        if stop_after < 1:
            raise ValueError("stop_after must be >= 1")
        if max_iters < 0 or leg_iters < 0:
            raise ValueError("max_iters and leg_iters must be >= 0")
        M = _pattern_of(H)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        self.per = None
        if per is not None:
            if isinstance(per, bool) or not isinstance(per, (float, np.floating)):
                raise TypeError("per must be a Float64")
            self.per = float(per)
            llr = llr_of_probs(np.full(self.n, self.per))
        elif channel_probs is not None:
            llr = llr_of_probs(channel_probs)
        else:
            llr = np.array(channel_llr, dtype=np.float32)
        if llr.shape != (self.n,):
            raise ValueError(f"one prior per bit: expected {self.n} entries, got shape {llr.shape}")
        self.channel_llr = np.ascontiguousarray(llr, dtype=np.float32)
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
        if np.float32(self.alpha) == 0.0 or np.float32(self.clip) == 0.0:
            # a zero in ldpc_relay_options selects the default there; here a default is spelled by leaving the keyword
            # out, so a zero gets the status the library gives every other value outside the range
            raise _capi.LdpcError(1, "alpha must lie in (0, 1] and clip must be finite and > 0 (got a zero)")
        self.scratch = MinSumScratchSpace(self.n)
        if device is None:
            device = _current_device()   # the current device NOW is the handle's for good (what info() answers)
        self.device = device
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64)
        opts = _capi.RelayOptions()
        opts.device = -1 if device is None else int(device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant, opts.stop_after = int(kernel_variant), stop_after
        self._h = ctypes.c_void_p()
        self._L = _capi.lib_for(None)
        _capi.check(self._L.ldpc_relay_create(self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                                              self.channel_llr.ctypes.data, legs, self.gammas.ctypes.data,
                                              self.leg_iters.ctypes.data, ctypes.byref(opts), ctypes.byref(self._h)), self._L)

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

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.ldpc_relay_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_batch_host(self, syn_bs, want_llr: bool = False, want_solutions: bool = False):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, llr [B][n] f64 | None, iters [B] i32), and with
        want_solutions a fifth entry: solutions [B] i32.  llr is the posterior as it stood when the syndrome stopped."""
        syn = np.ascontiguousarray(syn_bs, dtype=np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.s:
            raise AssertionError("syndrome length does not match the number of checks")
        B = int(syn.shape[0])
        err = np.empty((B, self.n), dtype=np.uint8)
        conv = np.empty(B, dtype=np.uint8)
        llr = np.empty((B, self.n), dtype=np.float64) if want_llr else None
        its = np.empty(B, dtype=np.int32)
        sol = np.empty(B, dtype=np.int32) if want_solutions else None
        _capi.check(self._L.ldpc_relay_decode_batch(self._h, B, syn.ctypes.data, err.ctypes.data, conv.ctypes.data,
                                                    llr.ctypes.data if want_llr else None, its.ctypes.data,
                                                    sol.ctypes.data if want_solutions else None), self._L)
        return (err, conv, llr, its, sol) if want_solutions else (err, conv, llr, its)

    def decode_batch_device(self, syn, err, conv, llr=None, iters=None, solutions=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, syn [B][s] u8, err [B][n] u8, conv [B] u8,
        llr [B][n] f64 | None, iters [B] i32 | None, solutions [B] i32 | None, all contiguous.  Asynchronous on `stream`
        (a hipStream_t as int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        for x in (syn, err, conv):
            assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        assert tuple(syn.shape) == (B, self.s) and tuple(err.shape) == (B, self.n) and conv.numel() == B
        if llr is not None:
            assert llr.is_cuda and llr.dtype == torch.float64 and llr.is_contiguous() and tuple(llr.shape) == (B, self.n)
        for x in (iters, solutions):
            if x is not None:
                assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and x.numel() == B
        if stream is None:
            stream = torch.cuda.current_stream(syn.device).cuda_stream
        _capi.check(self._L.ldpc_relay_decode_batch_device(
            self._h, B, syn.data_ptr(), err.data_ptr(), conv.data_ptr(), llr.data_ptr() if llr is not None else None,
            iters.data_ptr() if iters is not None else None, solutions.data_ptr() if solutions is not None else None,
            ctypes.c_void_p(stream)), self._L)

    def decode_(self, syndrome) -> Tuple[np.ndarray, bool]:
        """One syndrome: (scratch.err, converged); scratch.log_probabs holds its LLRs."""
        syn = syndrome_bytes(np.asarray(syndrome).reshape(-1))
        if syn.size != self.s:
            raise IndexError(f"syndrome has length {syn.size}, decoder has {self.s} checks")
        err, conv, llr, _ = self.decode_batch_host(syn.reshape(1, -1), want_llr=True)
        self.scratch.err[:] = err[0]
        self.scratch.log_probabs[:] = llr[0]
        return self.scratch.err, bool(conv[0])

    def batchdecode_(self, syndromes, errors, success=None):
        """syndromes s x B, errors n x B (overwritten), success [B]: one device call."""
        syndromes = np.asarray(syndromes)
        B = syndromes.shape[1]
        if success is None:
            success = np.empty(B, dtype=np.bool_)
        assert syndromes.shape[1] == errors.shape[1]
        assert syndromes.shape[1] == len(success)
        err, conv, llr, _ = self.decode_batch_host(np.ascontiguousarray(syndrome_bytes(syndromes).T), want_llr=True)
        errors[:, :] = err.T
        success[:] = conv.astype(np.bool_)
        if B > 0:
            self.scratch.err[:] = err[-1]
            self.scratch.log_probabs[:] = llr[-1]
        return errors, success
