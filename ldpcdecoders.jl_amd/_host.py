"""What the classes that own a library handle share: the handle's lifetime, the marshalling of a parity-check matrix, the
device a new handle takes, the checks on the arrays and tensors of a batch call, the reference's `decode!` /
`batchdecode!` pair over one host call, and the parsing of priors and options.  Nothing here touches a device."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import scipy.sparse as sp

from . import _capi


# ---- the handle -----------------------------------------------------------------------------------------------------------

class Handle:
    """An object that owns one handle `_h` of the library `_L`; `_destroy` names the function that frees it."""

    _destroy: str = ""
    _L = _h = None   # (until `_create` binds them: `close` and `__del__` are silent after a constructor that raised)

    def _create(self, L, create, *args) -> None:
        """`create(*args, &handle)` of the library L; the object owns the handle from here."""
        self._L = L
        h = ctypes.c_void_p()
        _capi.check(create(*args, ctypes.byref(h)), L)
        self._h = h

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            getattr(self._L, self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- matrices and devices ---------------------------------------------------------------------------------------------------

def _pattern_of(H) -> sp.csc_matrix:
    """`sparse(H)` (belief_propagation.jl:63): CSC pattern, rows ascending per column."""
    if sp.issparse(H):
        M = sp.csc_matrix(H, copy=True)
        M.sum_duplicates()
        M.eliminate_zeros()
    else:
        A = np.asarray(H)
        if A.ndim != 2:
            raise ValueError("H must be a matrix")
        M = sp.csc_matrix(A != 0)
    M.sort_indices()
    return M


def csc_arrays(M) -> Tuple[np.ndarray, np.ndarray]:
    """(colptr, rowval) of a CSC pattern as the int64 arrays a create call takes; the caller keeps them alive across it."""
    return np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int64)


def css_pattern(M) -> _capi.CSSPattern:
    """The ldpc_css_pattern of a CSC pattern; it keeps its two arrays alive itself."""
    colptr, rowval = csc_arrays(M)
    pat = _capi.CSSPattern(int(M.shape[0]), int(rowval.size), colptr.ctypes.data, rowval.ctypes.data)
    pat.arrays = (colptr, rowval)
    return pat


def current_device() -> Optional[int]:
    """torch's current GPU, or None without one or without torch (the create call then answers LDPC_ERR_NO_DEVICE
    itself).  A handle takes it at construction: the current device THEN is the handle's for good."""
    try:
        import torch

        return int(torch.cuda.current_device()) if torch.cuda.is_available() else None
    except Exception:
        return None


def device_option(device: Optional[int]) -> int:
    """The `device` field of an options structure: -1 = the library's choice."""
    return -1 if device is None else int(device)


# ---- the arrays and tensors of a batch call ---------------------------------------------------------------------------------

def syndrome_bytes(x) -> np.ndarray:
    """Map syndrome entries to the ABI's uint8 alphabet.

    0/1 (Bool, Int or integral Float) pass through.  Any other integer keeps
    its parity -- ``(-1)^x`` at belief_propagation.jl:136 only depends on it --
    and is encoded as 2 + parity so that it can never satisfy the ``==`` of the
    convergence test (:181), exactly like an Int 2 or 3 in the reference.
    A non-integral float is a DomainError in Julia; here a ValueError.
    """
    a = np.asarray(x)
    if a.dtype == np.bool_:
        return a.astype(np.uint8)
    if a.dtype == np.uint8 and (a.size == 0 or a.max() <= 1):
        return a
    if np.issubdtype(a.dtype, np.floating):
        if not np.all(np.isfinite(a)) or np.any(a != np.rint(a)):
            raise ValueError("syndrome entries must be integral ((-1)^x is a DomainError otherwise)")
        a = a.astype(np.int64)
    elif not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"unsupported syndrome element type {a.dtype}")
    a64 = a.astype(np.int64)
    out = np.where((a64 == 0) | (a64 == 1), a64, 2 + (a64 & 1))
    return out.astype(np.uint8)


def host_syndromes(syn_bs, s: int) -> np.ndarray:
    """[B][s] uint8, C-contiguous, of what a host entry is handed."""
    syn = np.ascontiguousarray(syn_bs, dtype=np.uint8)
    if syn.ndim != 2 or syn.shape[1] != s:
        raise AssertionError("syndrome length does not match the number of checks")
    return syn


def host_batch(syn_bs, s: int, n: int, want_llr: bool = False):
    """-> (syn, B, errors [B][n] u8, converged [B] u8, llr [B][n] f64 | None, iters [B] i32): the syndromes as
    `host_syndromes` gives them and the outputs of a host entry (uninitialised: the library writes every element)."""
    syn = host_syndromes(syn_bs, s)
    B = int(syn.shape[0])
    return (syn, B, np.empty((B, n), dtype=np.uint8), np.empty(B, dtype=np.uint8),
            np.empty((B, n), dtype=np.float64) if want_llr else None, np.empty(B, dtype=np.int32))


def host_ptr(a: Optional[np.ndarray]):
    return a.ctypes.data if a is not None else None


def tensor_ptr(x, dtype, shape, optional: bool = False):
    """The address of a device tensor after the check every device entry makes: a contiguous CUDA tensor of `dtype` and
    of `shape` (a tuple) or of `shape` elements (an int); AssertionError otherwise.  optional: None passes, as NULL."""
    if x is None and optional:
        return None
    assert x.is_cuda and x.dtype == dtype and x.is_contiguous(), (x.device, x.dtype, x.stride())
    assert x.numel() == shape if isinstance(shape, int) else tuple(x.shape) == tuple(shape), (tuple(x.shape), shape)
    return x.data_ptr()


def stream_ptr(stream: Optional[int], x) -> ctypes.c_void_p:
    """The hipStream_t a device entry runs on: `stream` as int, by default torch's current stream on the device of `x`."""
    if stream is None:
        import torch

        stream = torch.cuda.current_stream(x.device).cuda_stream
    return ctypes.c_void_p(stream)


# ---- decode! / batchdecode! over one host call --------------------------------------------------------------------------------

# For the decoders whose whole batch is one `decode_batch_host` call.  A class binds the two as its methods
# (`decode_ = _host.decode_`, in its own body: AbstractDecoder's placeholder comes first among its bases) and names in
# `_scratch_keeps` what `.scratch` holds of the last column afterwards: ("err", "log_probabs"), ("err",), or () -- then
# there is no scratch and `decode_` returns an Int copy.

def _whole_batch(decoder, syn_bs):
    """One host call -> (errors [B][n], converged [B], llr [B][n] | None)."""
    if "log_probabs" in decoder._scratch_keeps:
        return decoder.decode_batch_host(syn_bs, want_llr=True)[:3]
    return (*decoder.decode_batch_host(syn_bs)[:2], None)


def _keep_last(decoder, err, llr) -> None:
    if decoder._scratch_keeps:
        decoder.scratch.err[:] = err[-1]
    if llr is not None:
        decoder.scratch.log_probabs[:] = llr[-1]


def decode_(self, syndrome) -> Tuple[np.ndarray, bool]:
    """`decode!(decoder, syndrome)`: (scratch.err -- overwritten by the next call --, converged)."""
    syn = syndrome_bytes(np.asarray(syndrome).reshape(-1))
    if syn.size != self.s:
        raise IndexError(f"syndrome has length {syn.size}, decoder has {self.s} checks")
    err, conv, llr = _whole_batch(self, syn.reshape(1, -1))
    _keep_last(self, err, llr)
    return (self.scratch.err if self._scratch_keeps else err[0].astype(np.int64)), bool(conv[0])


def batchdecode_(self, syndromes, errors, success=None):
    """`batchdecode!(decoder, syndromes, errors, success)`: syndromes s x B, errors n x B (overwritten), success [B];
    one device call."""
    syndromes = np.asarray(syndromes)
    B = syndromes.shape[1]
    if success is None:
        success = np.empty(B, dtype=np.bool_)
    assert syndromes.shape[1] == errors.shape[1]
    assert syndromes.shape[1] == len(success)
    err, conv, llr = _whole_batch(self, np.ascontiguousarray(syndrome_bytes(syndromes).T))
    errors[:, :] = err.T
    success[:] = conv.astype(np.bool_)
    if B > 0:
        _keep_last(self, err, llr)
    return errors, success


# ---- priors and options -------------------------------------------------------------------------------------------------------

def as_int(x, name: str, note: str = "") -> int:
    """An `Int` argument of the reference's signatures: a bool or a float is a TypeError."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{name} must be an Int{note}")
    return int(x)


def llr_of_probs(probs) -> np.ndarray:
    """log(P(0) / P(1)) of error probabilities strictly inside (0, 1), as float32."""
    p = np.asarray(probs, dtype=np.float64)
    if p.size and not np.all((p > 0.0) & (p < 1.0)):   # (False for NaN as well)
        raise ValueError("probabilities must lie strictly inside (0, 1)")
    return np.log((1.0 - p) / p).astype(np.float32)


def one_prior_given(per, channel_probs, channel_llr) -> None:
    if (per is not None) + (channel_llr is not None) + (channel_probs is not None) != 1:
        raise TypeError("give exactly one of per, channel_probs and channel_llr")


def channel_prior(n: int, per=None, channel_probs=None, channel_llr=None) -> np.ndarray:
    """Exactly one of `per` (a Float64, the same for every bit), `channel_probs` (an error probability per bit) and
    `channel_llr` (log(P(0) / P(1)) per bit) -> the n prior LLRs as the float32 array handed to the library."""
    one_prior_given(per, channel_probs, channel_llr)
    if per is not None:
        if isinstance(per, bool) or not isinstance(per, (float, np.floating)):
            raise TypeError("per must be a Float64")
        llr = llr_of_probs(np.full(n, float(per)))
    elif channel_probs is not None:
        llr = llr_of_probs(channel_probs)
    else:
        llr = np.array(channel_llr, dtype=np.float32)
    if llr.shape != (n,):
        raise ValueError(f"one prior per bit: expected {n} entries, got shape {llr.shape}")
    return np.ascontiguousarray(llr, dtype=np.float32)


def refuse_zero_alpha_clip(alpha: float, clip: float) -> None:
    """A zero in an options structure selects the default there; in Python a default is spelled by leaving the keyword
    out, so a zero gets the status the library gives every other value outside the range."""
    if np.float32(alpha) == 0.0 or np.float32(clip) == 0.0:
        raise _capi.LdpcError(1, "alpha must lie in (0, 1] and clip must be finite and > 0 (got a zero)")
