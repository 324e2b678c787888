"""Joint Pauli min-sum decoder of a general (non-CSS) stabilizer code, over the ldpc_stab_minsum_* entry points (the rule
is stated in include/ldpc_mi355x_stab.h).  A code is a symplectic pair (Sx, Sz): stabilizer i has X or Y on qubit j where
Sx[i, j] is set, Z or Y where Sz[i, j] is set -- what a stabilizer tableau holds.  Every qubit carries the three beliefs of
`PauliMinSumDecoder` (X, Y, Z against I), every edge the Pauli type of its stabilizer there, so checks that mix X, Y and Z
(the five-qubit code, the XZZX surface code, a Clifford-deformed CSS code) are decoded jointly; on a CSS code -- Hx rows as
X-type, then Hz rows as Z-type -- the outputs equal `PauliMinSumDecoder`'s in every bit.  Not a decoder of the reference.
The syndrome s [B][r] is one bit per stabilizer: whether the error anticommutes with it, `Sx ez ^ Sz ex`.
`run_stabilizer_trials` is the Monte-Carlo loop around it; it adds no kernel: the CSS sampler draws the Pauli errors and
the binary scorer over [Sz | Sx] counts the failures."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np
import scipy.sparse as sp

from . import _capi, codes
from ._host import (Handle, _pattern_of, as_int, css_pattern, current_device, device_option, host_ptr, host_syndromes,
                    refuse_zero_alpha_clip, stream_ptr, tensor_ptr)
from .css_trials import CSSTrials, pauli_rates
from .pauli import pauli_priors
from .trials import TrialResult, Trials


def symplectic_syndromes(Sx, Sz, ex, ez) -> np.ndarray:
    """ex, ez [B][n] -> s [B][r] uint8: s = Sx ez ^ Sz ex (mod 2), whether each error anticommutes with each stabilizer."""
    return codes.syndromes_of(Sx, np.asarray(ez)) ^ codes.syndromes_of(Sz, np.asarray(ex))


class StabilizerMinSumDecoder(Handle):
    """`StabilizerMinSumDecoder(Sx, Sz, p, max_iters)`: `p` as `pauli_rates` takes it (a float: depolarizing noise of total
    rate p; a triple (px, py, pz)), the same for every qubit -- or `p=None` and `pauli_probs=` an (n, 3) array of per-qubit
    (px, py, pz): exactly one of the two.  alpha in (0, 1] scales every check-to-qubit message, clip > 0 clamps the
    qubit-to-check values.  kernel_variant: 0 = by size, 1 = on-chip, 2 = unlimited (`.kernel` tells which tier the handle
    takes).  check: assert Sx Sz' + Sz Sx' = 0 over GF(2), i.e. that the stabilizers commute (the library does not).
    Flooding schedule."""

    _destroy = "ldpc_stab_minsum_destroy"

    def __init__(self, Sx, Sz, p=None, max_iters: int = 50, alpha: float = 0.75, clip: float = 1e6, pauli_probs=None,
                 kernel_variant: int = 0, device: Optional[int] = None, check: bool = True):
        as_int(max_iters, "max_iters")
        if (p is None) == (pauli_probs is None):
            raise TypeError("give exactly one of p and pauli_probs")
        Mx, Mz = _pattern_of(Sx), _pattern_of(Sz)
        if Mx.shape != Mz.shape:
            raise AssertionError("Sx and Sz must have the same shape (one row per stabilizer, one column per qubit)")
        if check:
            A, B = Mx.astype(np.int64), Mz.astype(np.int64)
            prod = sp.csr_matrix(A @ B.T + B @ A.T)
            if (prod.data % 2).any():
                raise AssertionError("Sx * Sz' + Sz * Sx' != 0 over GF(2): the stabilizers do not commute")
        self.sparse_Sx, self.sparse_Sz = Mx, Mz
        self.n, self.rows = int(Mx.shape[1]), int(Mx.shape[0])
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
        opts = _capi.StabMinSumOptions()
        opts.device = device_option(self.device)
        opts.alpha, opts.clip = self.alpha, self.clip
        opts.kernel_variant = int(kernel_variant)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_stab_minsum_create, self.n, ctypes.byref(pat_x), ctypes.byref(pat_z), self.prior_x.ctypes.data,
                     self.prior_y.ctypes.data, self.prior_z.ctypes.data, self.max_iters, ctypes.byref(opts))

    @classmethod
    def from_paulis(cls, strings, *args, **kwargs):
        """From Pauli strings over I, X, Y, Z, one per stabilizer: `from_paulis(["XZZXI", "IXZZX", ...], p, max_iters)`."""
        Sx, Sz = codes.paulis_to_symplectic(strings)
        return cls(Sx, Sz, *args, **kwargs)

    @property
    def kernel(self) -> int:
        """1 = on-chip (state in LDS), 2 = unlimited (state in a global workspace) (ldpc_stab_minsum_kernel)."""
        return int(self._L.ldpc_stab_minsum_kernel(self._h))

    @property
    def tile_syndromes(self) -> int:
        """The syndromes a workgroup decodes at a time (S)."""
        return int(self._L.ldpc_stab_minsum_tile_syndromes(self._h))

    @property
    def last_grid(self) -> int:
        """The workgroups of the most recent launch (0 before any); fewer than ceil(batch / S): slots were reused."""
        return int(self._L.ldpc_stab_minsum_last_grid(self._h))

    def info(self):
        return SimpleNamespace(device=self.device, kernel=self.kernel, tile_syndromes=self.tile_syndromes, last_grid=self.last_grid)

    def decode_batch_host(self, s, want_llr: bool = False):
        """s [B][rows] uint8 (= Sx ez ^ Sz ex) -> (gx [B][n] u8, gz [B][n] u8, converged [B] u8, llr [B][3][n] f64 | None:
        the planes GX, GY, GZ, iters [B] i32)."""
        s = host_syndromes(s, self.rows)
        B = int(s.shape[0])
        gx, gz = np.empty((B, self.n), dtype=np.uint8), np.empty((B, self.n), dtype=np.uint8)
        conv = np.empty(B, dtype=np.uint8)
        llr = np.empty((B, 3, self.n), dtype=np.float64) if want_llr else None
        its = np.empty(B, dtype=np.int32)
        _capi.check(self._L.ldpc_stab_minsum_decode_batch(self._h, B, s.ctypes.data, gx.ctypes.data, gz.ctypes.data, conv.ctypes.data,
                                                          host_ptr(llr), its.ctypes.data), self._L)
        return gx, gz, conv, llr, its

    def decode_batch_device(self, s, gx, gz, conv, llr=None, iters=None, stream: Optional[int] = None) -> None:
        """HBM-resident batch: torch tensors on the decoder's GPU, s [B][rows], gx, gz [B][n], conv [B] u8, llr [B][3][n]
        f64 | None, iters [B] i32 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as int; default =
        torch's current stream)."""
        import torch

        B = int(s.shape[0])
        u8 = torch.uint8
        _capi.check(self._L.ldpc_stab_minsum_decode_batch_device(
            self._h, B, tensor_ptr(s, u8, (B, self.rows)), tensor_ptr(gx, u8, (B, self.n)), tensor_ptr(gz, u8, (B, self.n)),
            tensor_ptr(conv, u8, B), tensor_ptr(llr, torch.float64, (B, 3, self.n), optional=True),
            tensor_ptr(iters, torch.int32, B, optional=True), stream_ptr(stream, s)), self._L)


def run_stabilizer_trials(decoder, trials: int, p, batch: int = 65536, seed: int = 0, logicals=None) -> TrialResult:
    """`trials` Monte-Carlo trials of a `StabilizerMinSumDecoder` under Pauli noise `p` (a float: depolarizing; or a triple
    (px, py, pz)), in batches of `batch` (the last one ragged) on torch's current stream of the decoder's GPU.  No kernel of
    its own: a `CSSTrials` over (Sx, Sz) draws one Pauli per qubit and gives ex, ez, Sx ez and Sz ex, whose XOR is the
    syndrome; the decoder decodes it into (gx, gz); a binary `Trials` over [Sz | Sx] with the logical rows [LSz | LSx]
    scores cat(gx, gz) against cat(ex, ez): a block error (the guess differs from the error), a syndrome mismatch (the
    residual anticommutes with a stabilizer), a logical error (it anticommutes with a logical operator).  Trial number c is
    column c of the sampling rule, so the result does not depend on `batch`.  Only the four counts and the number of
    unconverged columns are read back.  logicals: None = `codes.stabilizer_logicals`, False = none, or a pair (LSx, LSz).
    Nothing here changes the decoder: whether its priors were built from the same `p` is the caller's choice."""
    import torch

    device = int(decoder.info().device) if decoder.info().device is not None else int(torch.cuda.current_device())
    dev = torch.device("cuda", device)
    total, batch = int(trials), int(batch)
    assert total >= 0 and batch > 0
    Sx, Sz = decoder.sparse_Sx, decoder.sparse_Sz
    if logicals is None:
        logicals = codes.stabilizer_logicals(Sx, Sz)
    rows = None if logicals is False else sp.hstack([_pattern_of(logicals[1]), _pattern_of(logicals[0])])
    sampler = CSSTrials(Sx, Sz, logicals=False, device=device, check=False)
    scorer = None
    try:
        scorer = Trials(sp.hstack([Sz, Sx]), rows, device=device)
        n, r = sampler.n, decoder.rows
        with torch.cuda.device(dev):
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            unconverged = torch.zeros((), dtype=torch.int64, device=dev)
            B = min(batch, max(total, 1))
            err, guess = (torch.empty((B, 2 * n), dtype=torch.uint8, device=dev) for _ in range(2))
            ex, ez, gx, gz = (torch.empty((B, n), dtype=torch.uint8, device=dev) for _ in range(4))
            sx, sz = (torch.empty((B, r), dtype=torch.uint8, device=dev) for _ in range(2))
            syn = torch.empty((B, r), dtype=torch.uint8, device=dev)
            conv = torch.empty(B, dtype=torch.uint8, device=dev)
            done = 0
            while done < total:
                b = min(B, total - done)
                sampler.sample(b, p, seed=seed, column0=done, out=(ex[:b], ez[:b], sx[:b], sz[:b]))
                torch.bitwise_xor(sx[:b], sz[:b], out=syn[:b])
                decoder.decode_batch_device(syn[:b], gx[:b], gz[:b], conv[:b])
                torch.cat((gx[:b], gz[:b]), dim=1, out=guess[:b])
                torch.cat((ex[:b], ez[:b]), dim=1, out=err[:b])
                scorer.score(guess[:b], err[:b], counts=counts, want_flags=False)
                unconverged += (conv[:b] == 0).sum()
                done += b
            c = counts.cpu().tolist()
            nc = int(unconverged.cpu())
    finally:
        sampler.close()
        if scorer is not None:
            scorer.close()
    return TrialResult(trials=int(c[0]), block_errors=int(c[1]), syndrome_mismatches=int(c[2]), logical_errors=int(c[3]),
                       not_converged=nc)
