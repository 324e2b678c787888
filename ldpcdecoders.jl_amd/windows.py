"""Sliding-window decoding of a detector error model: the plan (host, numpy), the window step on the device
(`WindowStep`, over the ldpc_windows_* entry points; the rule is stated in include/ldpc_mi355x.h) and
`SlidingWindowDecoder`, which chains any decoder of this package over the windows without leaving the GPU.

The plan.  `layers[d]` is the round of detector d, `first(j)` / `last(j)` the lowest / highest layer among the detectors
of mechanism j, R = max(layers) + 1.  Window k covers the layers [a_k, b_k), a_k = k * commit, b_k = min(a_k + width, R);
the window with b_k = R is the last.  det_k: the detectors of those layers; mech_k: the mechanisms with
a_k <= first(j) < b_k; the window decodes H[det_k, mech_k] (a column that reaches past b_k is truncated) at
rates[mech_k] and keeps -- commits -- the mechanisms with first(j) < a_k + commit, the last window all of its own.  So
every mechanism that has a detector is committed by exactly one window, and after the commit of window k every
uncommitted mechanism has all its detectors in layers >= a_{k+1}.  A mechanism without a detector is in no window and
its guess is 0."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._host import Handle, _pattern_of, csc_arrays, device_option, stream_ptr, syndrome_bytes, tensor_ptr
from ._host import current_device as _current_device
from .decoder import AbstractDecoder
from .dem import DetectorErrorModel


def phenomenological_layers(H, rounds: int) -> np.ndarray:
    """The layer of every detector of `phenomenological(H, logicals, rounds, p, q)`: detector t s + i is of round t."""
    R = int(rounds)
    if R < 1:
        raise ValueError("rounds must be >= 1")
    return np.repeat(np.arange(R, dtype=np.int64), int(_pattern_of(H).shape[0]))


@dataclass(frozen=True)
class Window:
    """Layers [a, b); `det` and `mech` ascending global indices; `commit` ascending positions in `mech`."""
    a: int
    b: int
    det: np.ndarray
    mech: np.ndarray
    commit: np.ndarray


class WindowPlan:
    """`.windows`: the `Window`s in order; `.uncovered`: the mechanisms in no window (no detector); `.sub_model(k)`: the
    model window k decodes."""

    def __init__(self, dem: DetectorErrorModel, layers: np.ndarray, width: int, commit: int, windows: List[Window],
                 uncovered: np.ndarray):
        self.dem, self.layers, self.width, self.commit = dem, layers, width, commit
        self.windows, self.uncovered = windows, uncovered

    def __len__(self) -> int:
        return len(self.windows)

    def sub_model(self, k: int) -> DetectorErrorModel:
        """H[det_k, mech_k], no observable rows, rates[mech_k]."""
        w = self.windows[k]
        return DetectorErrorModel(self.dem.H[w.det, :][:, w.mech], None, self.dem.rates[w.mech])


def window_plan(dem: DetectorErrorModel, layers, width: int, commit: int, strict: bool = True) -> WindowPlan:
    """The windows of `dem` by the rule of this module.  ValueError: width < 1, commit < 1, commit > width; `layers` not
    one non-negative integer per detector; and, under `strict`, a mechanism that a window other than the last would
    commit although it may reach past that window: last(j) - first(j) + 1 > width - commit + 1."""
    width, commit = int(width), int(commit)
    if width < 1 or commit < 1 or commit > width:
        raise ValueError("a window plan needs 1 <= commit <= width")
    lay = np.asarray(layers)
    D, N = dem.num_detectors, dem.num_mechanisms
    if lay.ndim != 1 or lay.shape[0] != D:
        raise ValueError(f"one layer per detector: expected {D} entries, got shape {lay.shape}")
    if D and not np.issubdtype(lay.dtype, np.integer):
        if not np.all(np.isfinite(lay)) or np.any(lay != np.rint(lay)):
            raise ValueError("layers must be whole numbers")
    lay = lay.astype(np.int64)
    if D and int(lay.min()) < 0:
        raise ValueError("layers must not be negative")
    R = int(lay.max()) + 1 if D else 0
    H = dem.H
    deg = np.diff(H.indptr)
    has = deg > 0
    first = np.full(N, -1, dtype=np.int64)
    last = np.full(N, -1, dtype=np.int64)
    if H.nnz:
        of_entry = lay[H.indices]
        starts = H.indptr[:-1][has]
        first[has] = np.minimum.reduceat(of_entry, starts)
        last[has] = np.maximum.reduceat(of_entry, starts)
    spans = []
    k = 0
    while R > 0:
        a, b = k * commit, min(k * commit + width, R)
        spans.append((a, b))
        if b == R:
            break
        k += 1
    if strict and len(spans) > 1:
        early = has & (first // commit < len(spans) - 1)           # committed by a window other than the last
        bad = np.flatnonzero(early & (last - first + 1 > width - commit + 1))
        if bad.size:
            j = int(bad[0])
            raise ValueError(f"mechanism {j} spans the layers {int(first[j])}..{int(last[j])}: more than width - commit + 1 = "
                             f"{width - commit + 1}, so a window would commit it while truncated (strict=False allows that)")
    windows = []
    for i, (a, b) in enumerate(spans):
        det = np.flatnonzero((lay >= a) & (lay < b)).astype(np.int64)
        mech = np.flatnonzero(has & (first >= a) & (first < b)).astype(np.int64)
        if i == len(spans) - 1:
            com = np.arange(mech.size, dtype=np.int64)
        else:
            com = np.flatnonzero(first[mech] < a + commit).astype(np.int64)
        windows.append(Window(a, b, det, mech, com))
    return WindowPlan(dem, lay, width, commit, windows, np.flatnonzero(~has).astype(np.int64))


def _lists(seqs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ptr [K + 1], idx) of a list of index lists, int64."""
    ptr = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in seqs], out=ptr[1:])
    idx = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in seqs]) if len(seqs) else np.zeros(0, dtype=np.int64)
    return ptr, np.ascontiguousarray(idx, dtype=np.int64)


class WindowStep(Handle):
    """The window step of `H` (D x N) on a device: `det[k]`, `mech[k]`, `commit[k]` (positions in mech[k]) for every window.
    `gather` and `commit` take contiguous uint8 torch tensors on that device and are asynchronous on `stream` (a
    hipStream_t as int; default torch's current stream)."""

    _destroy = "ldpc_windows_destroy"

    def __init__(self, H, det, mech, commit, device: Optional[int] = None):
        M = _pattern_of(H)
        self.D, self.N = int(M.shape[0]), int(M.shape[1])
        if not len(det) == len(mech) == len(commit):
            raise ValueError("one det, mech and commit list per window")
        self.ndet = [int(len(x)) for x in det]
        self.nmech = [int(len(x)) for x in mech]
        colptr, rowval = csc_arrays(M)
        lists = [a for seqs in (det, mech, commit) for a in _lists(seqs)]   # (ptr, idx) of each, kept alive across the call
        if device is None:
            device = _current_device()   # the current device NOW is the handle's for good
        opts = _capi.WindowsOptions()
        opts.device = device_option(device)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_windows_create, self.D, self.N, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, len(det),
                     *(a.ctypes.data for a in lists), ctypes.byref(opts))
        self.device = device

    def __len__(self) -> int:
        return int(self._L.ldpc_windows_count(self._h))

    def gather(self, k: int, residual, out=None, stream: Optional[int] = None):
        """residual [B][D] -> window k's syndromes [B][|det_k|]."""
        import torch

        k, B = int(k), int(residual.shape[0])
        if out is None:
            out = torch.empty((B, self.ndet[k]), dtype=torch.uint8, device=residual.device)
        _capi.check(self._L.ldpc_windows_gather_device(self._h, k, B, tensor_ptr(residual, torch.uint8, (B, self.D)),
                                                       tensor_ptr(out, torch.uint8, (B, self.ndet[k])), stream_ptr(stream, residual)),
                    self._L)
        return out

    def commit(self, k: int, win_guess, residual, guess, win_conv=None, conv=None, next_syndromes=None,
               stream: Optional[int] = None) -> None:
        """Window k's guess [B][|mech_k|] into guess [B][N] and residual [B][D]; the flags [B] and the next window's
        syndromes [B][|det_{k+1}|] where given."""
        import torch

        k, B, u8 = int(k), int(residual.shape[0]), torch.uint8
        _capi.check(self._L.ldpc_windows_commit_device(
            self._h, k, B, tensor_ptr(win_guess, u8, (B, self.nmech[k])), tensor_ptr(win_conv, u8, (B,), optional=True),
            tensor_ptr(residual, u8, (B, self.D)), tensor_ptr(guess, u8, (B, self.N)), tensor_ptr(conv, u8, (B,), optional=True),
            tensor_ptr(next_syndromes, u8, (B, self.ndet[k + 1])) if next_syndromes is not None else None,   # (no k + 1 after the last)
            stream_ptr(stream, residual)), self._L)


class SlidingWindowDecoder(AbstractDecoder):
    """`dem` decoded window by window (`window_plan(dem, layers, width, commit, strict)`): `make_decoder(sub_model)` returns
    the decoder of a window's model -- any decoder `run_trials` drives, e.g.
    `lambda m: MinSumDecoder(m.H, None, 30, channel_probs=m.rates)` -- and is called once per DISTINCT window model
    (equal shape, pattern and rates share a decoder: `.decoders`, `.window_decoder[k]`).  A column's flag is the AND of
    its windows' flags.  With width >= R there is one window, the model itself."""

    def __init__(self, dem: DetectorErrorModel, layers, width: int, commit: int, make_decoder: Callable, strict: bool = True,
                 device: Optional[int] = None):
        import torch

        self.plan = window_plan(dem, layers, width, commit, strict)
        self.sparse_H = dem.H
        self.per = None
        self.s, self.n = dem.num_detectors, dem.num_mechanisms
        if device is None:
            device = _current_device()
        self.device = device
        self.decoders, self.window_decoder = [], []
        self._step = None
        self._cap, self._res = 0, None
        self.residual = None
        seen = {}
        try:
            for k in range(len(self.plan)):
                m = self.plan.sub_model(k)
                key = (m.H.shape, m.H.indptr.astype(np.int64).tobytes(), m.H.indices.astype(np.int64).tobytes(), m.rates.tobytes())
                if key not in seen:
                    seen[key] = len(self.decoders)
                    if device is None:
                        self.decoders.append(make_decoder(m))   # (no GPU: the decoder's create says so)
                    else:
                        with torch.cuda.device(int(device)):
                            self.decoders.append(make_decoder(m))
                self.window_decoder.append(seen[key])
            w = self.plan.windows
            self._step = WindowStep(dem.H, [x.det for x in w], [x.mech for x in w], [x.commit for x in w], device=device)
        except Exception:
            self.close()
            raise
        self._max_det = max([x.det.size for x in w], default=0)
        self._max_mech = max([x.mech.size for x in w], default=0)
        self._uncovered = None

    def info(self):
        """`.device`: the GPU of the window step; `.windows`, `.decoders`: how many of each."""
        return SimpleNamespace(device=self.device, windows=len(self.plan), decoders=len(self.decoders))

    def close(self) -> None:
        for d in getattr(self, "decoders", []):
            if hasattr(d, "close"):          # (BeliefPropagationOSDDecoder has none: its parts free themselves)
                d.close()
        self.decoders = []
        step, self._step = getattr(self, "_step", None), None
        if step is not None:
            step.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _grow(self, B: int, dev) -> None:
        """The buffers of the handle: the residual, two windows' syndromes (this one's and the next one's), a window's
        guess and flags.  Kept between calls, regrown (on the stream, by torch's allocator) when a batch is larger."""
        import torch

        if self._res is not None and B <= self._cap and self._res.device == dev:
            return
        B = max(B, 1)
        self._res = torch.empty((B, self.s), dtype=torch.uint8, device=dev)
        self._wsyn = [torch.empty(B * self._max_det, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._wguess = torch.empty(B * self._max_mech, dtype=torch.uint8, device=dev)
        self._wconv = torch.empty(B, dtype=torch.uint8, device=dev)
        if self._uncovered is None or self._uncovered.device != dev:
            self._uncovered = torch.from_numpy(self.plan.uncovered).to(dev)
        self._cap, self._stream = B, torch.cuda.current_stream(dev)

    def decode_batch_device(self, syn, err, conv, stream: Optional[int] = None) -> None:
        """HBM-resident batch: syn [B][s] u8, err [B][n] u8, conv [B] u8, contiguous torch tensors on the decoder's GPU.
        Everything runs on `stream` (a hipStream_t as int; default torch's current stream) without a host synchronisation
        of this layer's own; `.residual` is syn ^ H * err afterwards (for 0/1 syndromes)."""
        import torch

        B = int(syn.shape[0])
        for x, shape in ((syn, (B, self.s)), (err, (B, self.n)), (conv, B)):
            tensor_ptr(x, torch.uint8, shape)
        if stream is not None and int(stream) != torch.cuda.current_stream(syn.device).cuda_stream:
            # the window decoders are driven on torch's current stream: make `stream` that one
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=syn.device)):
                return self.decode_batch_device(syn, err, conv)
        from .trials import _device_decode

        with torch.cuda.device(syn.device):
            self._grow(B, syn.device)
            if torch.cuda.current_stream(syn.device) != self._stream:
                # used on another stream than the one they were allocated on: torch's allocator must know before a regrow frees them
                for t in (self._res, self._wguess, self._wconv, *self._wsyn):
                    t.record_stream(torch.cuda.current_stream(syn.device))
            res = self.residual = self._res[:B]
            res.copy_(syn)
            if self._uncovered.numel():
                err[:, self._uncovered] = 0
            K = len(self.plan)
            if K == 0 or B == 0:
                conv.fill_(1)
                return
            w = self.plan.windows
            wsyn = self._wsyn[0][:B * w[0].det.size].view(B, w[0].det.size)
            self._step.gather(0, res, out=wsyn)
            for k in range(K):
                nm = w[k].mech.size
                wguess, wconv = self._wguess[:B * nm].view(B, nm), self._wconv[:B]
                guesses = _device_decode(self.decoders[self.window_decoder[k]], wsyn, wguess, wconv, 0)
                nxt = None
                if k + 1 < K:
                    nd = w[k + 1].det.size
                    nxt = self._wsyn[(k + 1) & 1][:B * nd].view(B, nd)
                self._step.commit(k, guesses, res, err, win_conv=wconv, conv=conv.view(B), next_syndromes=nxt)
                wsyn = nxt

    def decode_batch_host(self, syn_bs):
        """syn [B][s] uint8 -> (errors [B][n] u8, converged [B] u8, residual [B][s] u8)."""
        import torch

        syn = np.ascontiguousarray(syn_bs, dtype=np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.s:
            raise AssertionError("syndrome length does not match the number of detectors")
        B = int(syn.shape[0])
        dev = torch.device("cuda", int(self.device))
        d_syn = torch.from_numpy(syn).to(dev)
        err = torch.empty((B, self.n), dtype=torch.uint8, device=dev)
        conv = torch.empty(B, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            self.decode_batch_device(d_syn, err, conv)
            return err.cpu().numpy(), conv.cpu().numpy(), self.residual.cpu().numpy()

    def decode_(self, syndrome) -> Tuple[np.ndarray, bool]:
        """One syndrome: (guess as Float64 0.0 / 1.0, every window converged)."""
        syn = syndrome_bytes(np.asarray(syndrome).reshape(-1))
        if syn.size != self.s:
            raise IndexError(f"syndrome has length {syn.size}, decoder has {self.s} detectors")
        err, conv, _ = self.decode_batch_host(syn.reshape(1, -1))
        return err[0].astype(np.float64), bool(conv[0])

    def batchdecode_(self, syndromes, errors, success=None):
        """syndromes s x B, errors n x B (overwritten), success [B]."""
        syndromes = np.asarray(syndromes)
        B = syndromes.shape[1]
        if success is None:
            success = np.empty(B, dtype=np.bool_)
        assert syndromes.shape[1] == errors.shape[1]
        assert syndromes.shape[1] == len(success)
        err, conv, _ = self.decode_batch_host(np.ascontiguousarray(syndrome_bytes(syndromes).T))
        errors[:, :] = err.T
        success[:] = conv.astype(np.bool_)
        return errors, success
