"""Monte-Carlo trials of a CSS code on the device, over the ldpc_css_trials_* entry points: Pauli errors on n qubits
(depolarizing or biased; one draw per qubit gives its X part `ex` and its Z part `ez`, so a Y error exists), the two
syndromes `sz = Hz ex` and `sx = Hx ez`, and a joint score that counts logical X and logical Z failures.  The rules
are stated in include/ldpc_mi355x.h; `run_css_trials` loops sample -> two decoders' device entries -> score and reads
back the six counts and the two numbers of unconverged columns."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi, codes
from ._host import Handle, _pattern_of, css_pattern, current_device, device_option, stream_ptr, tensor_ptr
from .trials import _M64, _device_decode


def pauli_rates(p):
    """`p` -> (px, py, pz): a float is depolarizing noise of total rate p (px = py = pz = p / 3), a triple is itself."""
    if isinstance(p, (tuple, list, np.ndarray)):
        px, py, pz = (float(x) for x in p)
        return px, py, pz
    return (float(p) / 3.0,) * 3


def conditional_probs(p):
    """(p_if0, p_if1): the probability that a qubit's Z part is flipped given that its X part is not / is, under Pauli
    noise `p` (as `pauli_rates` takes it), in float64.  An X part is an X or a Y and only the Y carries a Z part, so
    p_if1 = py / (px + py); without an X part the qubit holds I or Z: p_if0 = pz / (1 - px - py).  ValueError where
    either is not strictly inside (0, 1) -- px + py = 0 included."""
    px, py, pz = (np.float64(x) for x in pauli_rates(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        p_if1 = py / (px + py)
        p_if0 = pz / (np.float64(1.0) - px - py)
    for name, v in (("p_if0", p_if0), ("p_if1", p_if1)):
        if not (0.0 < v < 1.0):   # (False for NaN as well)
            raise ValueError(f"{name} = {v} is not strictly inside (0, 1) for the rates {(float(px), float(py), float(pz))}")
    return float(p_if0), float(p_if1)


class CSSTrials(Handle):
    """Owns the Tanner graphs of `Hx`, `Hz` and of the logical rows on a device.  logicals: None = `codes.css_logicals`,
    False = no logical rows (flag bits 2 and 3 are then never set), or a pair (Lx, Lz).  check: assert Hx * Hz' = 0
    over GF(2) (the library does not).  kernel_variant: 0 = by size, 1 = on-chip bit images, 2 = unlimited (`.kernel`
    tells which one the handle takes)."""

    _destroy = "ldpc_css_trials_destroy"

    def __init__(self, Hx, Hz, logicals=None, device: Optional[int] = None, kernel_variant: int = 0, check: bool = True):
        Mx, Mz = _pattern_of(Hx), _pattern_of(Hz)
        if int(Mx.shape[1]) != int(Mz.shape[1]):
            raise AssertionError("Hx and Hz must have the same number of columns")
        if check:
            prod = Mx.astype(np.int64) @ Mz.astype(np.int64).T
            if (prod.data % 2).any():
                raise AssertionError("Hx * Hz' != 0 over GF(2): the X and Z checks do not commute")
        self.n, self.rows_x, self.rows_z = int(Mx.shape[1]), int(Mx.shape[0]), int(Mz.shape[0])
        if logicals is None:
            logicals = codes.css_logicals(Mx, Mz)
        mats = [Mx, Mz]
        if logicals is not False:
            Lx, Lz = logicals
            for L in (Lx, Lz):
                Lm = _pattern_of(L)
                if int(Lm.shape[1]) != self.n:
                    raise AssertionError("logicals must have as many columns as Hx and Hz")
                mats.append(Lm)
        self.nlx = int(mats[2].shape[0]) if len(mats) > 2 else 0
        self.nlz = int(mats[3].shape[0]) if len(mats) > 3 else 0
        pats = [css_pattern(M) for M in mats]
        refs = [ctypes.byref(pat) for pat in pats] + [None] * (4 - len(pats))
        if device is None:
            device = current_device()   # (the current device NOW is the handle's for good, as in Trials)
        opts = _capi.CSSTrialsOptions()
        opts.device = device_option(device)
        opts.kernel_variant = int(kernel_variant)
        L = _capi.lib_for(None)
        self._create(L, L.ldpc_css_trials_create, self.n, *refs, ctypes.byref(opts))
        self.device = device

    @property
    def kernel(self) -> int:
        """1 = on-chip bit images, 2 = unlimited (ldpc_css_trials_kernel)."""
        return int(self._L.ldpc_css_trials_kernel(self._h))

    def _torch_device(self):
        import torch

        return torch.device("cuda", int(self.device))

    # -- device forms (torch tensors, asynchronous on `stream`: a hipStream_t as int, default torch's current stream) --
    def sample(self, batch: int, p, seed: int = 0, column0: int = 0, out=None, stream: Optional[int] = None):
        """-> (ex [batch][n], ez [batch][n], sx [batch][rows_x], sz [batch][rows_z]), all u8.  `out` = (ex, ez, sx, sz) to
        write into; None for both sx and sz there skips the syndromes (errors only)."""
        import torch

        B = int(batch)
        px, py, pz = pauli_rates(p)
        if out is None:
            dev = self._torch_device()
            ex, ez = (torch.empty((B, self.n), dtype=torch.uint8, device=dev) for _ in range(2))
            sx = torch.empty((B, self.rows_x), dtype=torch.uint8, device=dev)
            sz = torch.empty((B, self.rows_z), dtype=torch.uint8, device=dev)
        else:
            ex, ez, sx, sz = out
        u8 = torch.uint8
        _capi.check(self._L.ldpc_css_trials_sample_device(
            self._h, B, int(column0), px, py, pz, int(seed) & _M64, tensor_ptr(ex, u8, (B, self.n)), tensor_ptr(ez, u8, (B, self.n)),
            tensor_ptr(sx, u8, (B, self.rows_x), optional=True), tensor_ptr(sz, u8, (B, self.rows_z), optional=True),
            stream_ptr(stream, ex)), self._L)
        return ex, ez, sx, sz

    def syndromes(self, ex, ez, out=None, stream: Optional[int] = None):
        """ex, ez [B][n] u8 -> (sx [B][rows_x], sz [B][rows_z]) u8: sx = Hx ez, sz = Hz ex (mod 2)."""
        import torch

        B = int(ex.shape[0])
        if out is None:
            sx = torch.empty((B, self.rows_x), dtype=torch.uint8, device=ex.device)
            sz = torch.empty((B, self.rows_z), dtype=torch.uint8, device=ex.device)
        else:
            sx, sz = out
        u8 = torch.uint8
        _capi.check(self._L.ldpc_css_trials_syndromes_device(
            self._h, B, tensor_ptr(ex, u8, (B, self.n)), tensor_ptr(ez, u8, (B, self.n)), tensor_ptr(sx, u8, (B, self.rows_x)),
            tensor_ptr(sz, u8, (B, self.rows_z)), stream_ptr(stream, ex)), self._L)
        return sx, sz

    def score(self, gx, gz, ex, ez, flags=None, counts=None, stream: Optional[int] = None, want_flags: bool = True):
        """gx, gz, ex, ez [B][n] u8 -> (flags [B] u8, counts [6] i64).  `counts` is ACCUMULATED into (a fresh one starts
        at zero): trials, columns with dx or dz != 0, with a syndrome mismatch, with a logical failure, with a logical
        X failure, with a logical Z failure.  want_flags=False: no flags."""
        import torch

        B = int(ex.shape[0])
        ptrs = [tensor_ptr(x, torch.uint8, (B, self.n)) for x in (gx, gz, ex, ez)]
        if flags is None and want_flags:
            flags = torch.empty(B, dtype=torch.uint8, device=ex.device)
        if counts is None:
            counts = torch.zeros(6, dtype=torch.int64, device=ex.device)
        _capi.check(self._L.ldpc_css_trials_score_device(self._h, B, *ptrs, tensor_ptr(flags, torch.uint8, B, optional=True),
                                                         tensor_ptr(counts, torch.int64, 6), stream_ptr(stream, ex)), self._L)
        return flags, counts

    # -- host forms (numpy, synchronous) ---------------------------------------------------------------------------
    def sample_host(self, batch: int, p, seed: int = 0, column0: int = 0):
        B = int(batch)
        px, py, pz = pauli_rates(p)
        ex, ez = np.empty((B, self.n), dtype=np.uint8), np.empty((B, self.n), dtype=np.uint8)
        sx, sz = np.empty((B, self.rows_x), dtype=np.uint8), np.empty((B, self.rows_z), dtype=np.uint8)
        _capi.check(self._L.ldpc_css_trials_sample(self._h, B, int(column0), px, py, pz, int(seed) & _M64, ex.ctypes.data,
                                                   ez.ctypes.data, sx.ctypes.data, sz.ctypes.data), self._L)
        return ex, ez, sx, sz

    def score_host(self, gx, gz, ex, ez, counts=None):
        """-> (flags [B] u8, counts [6] i64); `counts` (numpy int64[6]) is accumulated into."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in (gx, gz, ex, ez)]
        B = int(arrs[2].shape[0])
        assert all(a.shape == (B, self.n) for a in arrs)
        flags = np.empty(B, dtype=np.uint8)
        if counts is None:
            counts = np.zeros(6, dtype=np.int64)
        assert counts.dtype == np.int64 and counts.flags.c_contiguous and counts.size == 6
        _capi.check(self._L.ldpc_css_trials_score(self._h, B, *(a.ctypes.data for a in arrs), flags.ctypes.data, counts.ctypes.data),
                    self._L)
        return flags, counts


@dataclass
class CSSTrialResult:
    trials: int
    block_errors: int            # gx != ex or gz != ez
    syndrome_mismatches: int     # a guess does not reproduce its error's syndrome
    logical_errors: int          # a logical X or a logical Z failure
    logical_x_errors: int        # Lz * (gx ^ ex) != 0
    logical_z_errors: int        # Lx * (gz ^ ez) != 0
    not_converged_hx: int        # columns whose decoder on Hx reported false
    not_converged_hz: int        # the same for the decoder on Hz

    def _rate(self, k: int) -> float:
        return k / self.trials if self.trials else 0.0

    @property
    def block_error_rate(self) -> float:
        return self._rate(self.block_errors)

    @property
    def syndrome_mismatch_rate(self) -> float:
        return self._rate(self.syndrome_mismatches)

    @property
    def logical_error_rate(self) -> float:
        return self._rate(self.logical_errors)

    @property
    def logical_x_error_rate(self) -> float:
        return self._rate(self.logical_x_errors)

    @property
    def logical_z_error_rate(self) -> float:
        return self._rate(self.logical_z_errors)

    @property
    def not_converged_hx_rate(self) -> float:
        return self._rate(self.not_converged_hx)

    @property
    def not_converged_hz_rate(self) -> float:
        return self._rate(self.not_converged_hz)


def _bp_of(decoder):
    from .osd import BeliefPropagationOSDDecoder

    return decoder.bp_decoder if isinstance(decoder, BeliefPropagationOSDDecoder) else decoder


def run_css_trials(decoder_hx, decoder_hz, trials: int, p, batch: int = 65536, seed: int = 0, logicals=None,
                   correlated: bool = False) -> CSSTrialResult:
    """`trials` Monte-Carlo trials of a CSS code under Pauli noise `p` (a float: depolarizing, px = py = pz = p / 3; or a
    triple (px, py, pz)).  `decoder_hz` (BP, BP+OSD, BP-OTS or bit-flip, built on Hz) decodes sz = Hz ex into the guess
    gx; `decoder_hx` (built on Hx) decodes sx = Hx ez into gz.  sample -> decode -> decode -> score run in batches of
    `batch` (the last one ragged) on torch's current stream of the decoders' GPU; trial number c is column c of the
    sampling rule (and of the bit-flip tie rule), so the result does not depend on `batch`.  Only the six counts and
    the two numbers of unconverged columns are read back.  logicals: as in CSSTrials.

    correlated=False: each decoder sees one side of the noise only.  Under depolarizing noise of total rate p, the
    marginal rate of either side is 2 p / 3 (an X part is an X or a Y); whether the decoders are built with that `per`
    is the caller's choice: nothing here changes a decoder.

    correlated=True: the two sides are decoded one after the other, because a Y error hits both.  `decoder_hz` decodes sz
    into gx as before; `decoder_hx` -- which must be a `MinSumDecoder` of either schedule -- then decodes sx with the
    prior of every qubit chosen by that guess: `conditional_probs(p)` gives P(Z part | X part not flipped / flipped), and
    `decode_batch_given_device(sx, gx, ...)` selects between the two per trial and qubit on the device.  The logical-X
    count is that of the uncorrelated run by construction.  The function sets the two tables on `decoder_hx`
    (`set_conditional_priors`) once from `p`: that is the one thing it changes on a decoder; the prior `decoder_hx` was
    built with plays no part."""
    import torch

    if correlated:
        from .minsum import MinSumDecoder

        if not isinstance(decoder_hx, MinSumDecoder):
            raise TypeError("correlated=True needs a MinSumDecoder as decoder_hx (only it has an entry with per-syndrome "
                            f"priors), got {type(decoder_hx).__name__}")
        p_if0, p_if1 = conditional_probs(p)
        decoder_hx.set_conditional_priors(probs_if0=p_if0, probs_if1=p_if1)
    bx, bz = _bp_of(decoder_hx), _bp_of(decoder_hz)
    devices = [int(b.info().device) if hasattr(b, "info") else int(torch.cuda.current_device()) for b in (bx, bz)]
    assert devices[0] == devices[1], f"the two decoders live on different GPUs ({devices[0]} and {devices[1]})"
    assert int(bx.sparse_H.shape[1]) == int(bz.sparse_H.shape[1]), "decoder_hx and decoder_hz must have the same number of bits"
    device = devices[1]
    dev = torch.device("cuda", int(device))
    total, batch = int(trials), int(batch)
    assert total >= 0 and batch > 0
    tr = CSSTrials(bx.sparse_H, bz.sparse_H, logicals, device=int(device))
    try:
        with torch.cuda.device(dev):
            counts = torch.zeros(6, dtype=torch.int64, device=dev)
            unconverged = torch.zeros(2, dtype=torch.int64, device=dev)
            B = min(batch, max(total, 1))
            ex, ez, gx, gz = (torch.empty((B, tr.n), dtype=torch.uint8, device=dev) for _ in range(4))
            sx = torch.empty((B, tr.rows_x), dtype=torch.uint8, device=dev)
            sz = torch.empty((B, tr.rows_z), dtype=torch.uint8, device=dev)
            cx, cz = torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
            done = 0
            while done < total:
                b = min(B, total - done)
                tr.sample(b, p, seed=seed, column0=done, out=(ex[:b], ez[:b], sx[:b], sz[:b]))
                guess_x = _device_decode(decoder_hz, sz[:b], gx[:b], cz[:b], done)
                if correlated:
                    decoder_hx.decode_batch_given_device(sx[:b], guess_x, gz[:b], cx[:b])
                    guess_z = gz[:b]
                else:
                    guess_z = _device_decode(decoder_hx, sx[:b], gz[:b], cx[:b], done)
                tr.score(guess_x, guess_z, ex[:b], ez[:b], counts=counts, want_flags=False)
                unconverged[0] += (cx[:b] == 0).sum()
                unconverged[1] += (cz[:b] == 0).sum()
                done += b
            c = counts.cpu().tolist()
            nc = unconverged.cpu().tolist()
    finally:
        tr.close()
    return CSSTrialResult(trials=int(c[0]), block_errors=int(c[1]), syndrome_mismatches=int(c[2]), logical_errors=int(c[3]),
                          logical_x_errors=int(c[4]), logical_z_errors=int(c[5]), not_converged_hx=int(nc[0]),
                          not_converged_hz=int(nc[1]))


def run_css_joint_trials(decoder, trials: int, p, batch: int = 65536, seed: int = 0, logicals=None) -> CSSTrialResult:
    """`run_css_trials` with ONE joint decoder in place of the two binary ones: `decoder` is a `PauliMinSumDecoder` built
    on (Hx, Hz); every batch is sampled under Pauli noise `p`, decoded once from (sx, sz) into (gx, gz), and scored, all
    on torch's current stream of the decoder's GPU.  Trial number c is column c of the sampling rule, so the result does
    not depend on `batch`.  Only the six counts and the number of unconverged columns are read back; a joint decode
    converges or not as a whole, so `not_converged_hx` and `not_converged_hz` both hold that number.  Nothing here
    changes the decoder: whether its priors were built from the same `p` is the caller's choice.  logicals: as in
    CSSTrials."""
    import torch

    device = int(decoder.info().device) if decoder.info().device is not None else int(torch.cuda.current_device())
    dev = torch.device("cuda", device)
    total, batch = int(trials), int(batch)
    assert total >= 0 and batch > 0
    tr = CSSTrials(decoder.sparse_Hx, decoder.sparse_Hz, logicals, device=device)
    try:
        with torch.cuda.device(dev):
            counts = torch.zeros(6, dtype=torch.int64, device=dev)
            unconverged = torch.zeros(1, dtype=torch.int64, device=dev)
            B = min(batch, max(total, 1))
            ex, ez, gx, gz = (torch.empty((B, tr.n), dtype=torch.uint8, device=dev) for _ in range(4))
            sx = torch.empty((B, tr.rows_x), dtype=torch.uint8, device=dev)
            sz = torch.empty((B, tr.rows_z), dtype=torch.uint8, device=dev)
            conv = torch.empty(B, dtype=torch.uint8, device=dev)
            done = 0
            while done < total:
                b = min(B, total - done)
                tr.sample(b, p, seed=seed, column0=done, out=(ex[:b], ez[:b], sx[:b], sz[:b]))
                decoder.decode_batch_device(sx[:b], sz[:b], gx[:b], gz[:b], conv[:b])
                tr.score(gx[:b], gz[:b], ex[:b], ez[:b], counts=counts, want_flags=False)
                unconverged[0] += (conv[:b] == 0).sum()
                done += b
            c = counts.cpu().tolist()
            nc = int(unconverged.cpu().tolist()[0])
    finally:
        tr.close()
    return CSSTrialResult(trials=int(c[0]), block_errors=int(c[1]), syndrome_mismatches=int(c[2]), logical_errors=int(c[3]),
                          logical_x_errors=int(c[4]), logical_z_errors=int(c[5]), not_converged_hx=nc, not_converged_hz=nc)
