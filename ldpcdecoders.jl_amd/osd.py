"""BP+OSD decoder: host mirror of `BeliefPropagationOSDDecoder`
(src/decoders/belief_propagation_osd.jl:17-29, 49-61).

BP runs on the MI355X (the hot path); the ordered-statistics step is host code inside
libldpc_mi355x.so (`ldpc_osd_postprocess_batch`, bit-packed GF(2) elimination threaded over
the batch) -- BASELINE config 5 asks for exactly that split ("BP+OSD post-processing on host").

Opt-in (`osd="device"`): the same step as HIP kernels (`ldpc_osd_postprocess_batch_device`), for batches
that should not leave the GPU.  Its reliability key is the stated one (include/ldpc_mi355x.h: pm_exp, ties by
column index); on the rare syndrome where libm's exp orders two nearly tied columns the other way round, it
returns another, equally valid estimate than the host form.

A second rule, opt-in and device form only (`method=` / `osd_method=`; include/ldpc_mi355x.h "THE STANDARD RULE"): the
columns most likely in error are eliminated first, the search is exhaustive or the combination sweep, and the cost of a
correction is an integer weight per bit (all ones, or from channel LLRs).  The reference's rule stays the default.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import _capi
from ._host import Handle, _pattern_of, csc_arrays, device_option, stream_ptr, syndrome_bytes, tensor_ptr
from .decoder import AbstractDecoder, BeliefPropagationDecoder


OSD_METHODS = {"reference": 0, "exhaustive": 1, "combination_sweep": 2}


class OSDPostProcessor(Handle):
    """Owns the `ldpc_osd` handle: bit-packed H and the OSD order.  Needs no GPU.
    method: "reference" (the reference's rule: host and device form), or "exhaustive" / "combination_sweep" (the
    standard rule, ldpc_osd_set_search: device form only).  weights: an array of n channel LLRs for the standard rule's
    cost (None: the Hamming weight)."""

    _destroy = "ldpc_osd_destroy"

    def __init__(self, H, osd_order: int = 0, method: str = "reference", weights=None):
        if method not in OSD_METHODS:
            raise ValueError('method must be "reference", "exhaustive" or "combination_sweep"')
        M = _pattern_of(H)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.osd_order = int(osd_order)
        self.method = method
        if weights is not None:
            if method == "reference":
                raise ValueError("the reference rule weighs by count: weights= needs another method")
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            if weights.shape != (self.n,):
                raise ValueError(f"weights must hold one channel LLR per bit ({self.n}), got shape {weights.shape}")
        colptr, rowval = csc_arrays(M)
        L = _capi.lib()
        # (ldpc_osd_create bounds the reference rule's order; ldpc_osd_set_search sets and bounds the standard rule's)
        self._create(L, L.ldpc_osd_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.osd_order if method == "reference" else 0)
        if method != "reference":
            _capi.check(L.ldpc_osd_set_search(self._h, OSD_METHODS[method], self.osd_order, self.n,
                                              None if weights is None else weights.ctypes.data), L)

    def postprocess(self, syn_bs, bp_err_bn, llr_bn, nthreads: int = 0) -> np.ndarray:
        """syn [B][s] u8 (0/1), bp_err [B][n] u8, llr [B][n] f64 -> errors [B][n] u8."""
        syn = np.ascontiguousarray(syn_bs, dtype=np.uint8)
        e = np.ascontiguousarray(bp_err_bn, dtype=np.uint8)
        L = np.ascontiguousarray(llr_bn, dtype=np.float64)
        B = syn.shape[0]
        assert syn.shape == (B, self.s) and e.shape == (B, self.n) and L.shape == (B, self.n)
        out = np.empty((B, self.n), dtype=np.uint8)
        _capi.check(self._L.ldpc_osd_postprocess_batch(self._h, B, syn.ctypes.data, e.ctypes.data,
                                                       L.ctypes.data, out.ctypes.data, int(nthreads)), self._L)
        return out

    # -- the opt-in device form ------------------------------------------------
    def prepare_device(self, device=None, kernel_variant: int = 0) -> int:
        """Upload the packed rows to `device` (None: the current one) and pick the kernel tier (0: by size; 1..3
        force it).  Once per post-processor.  Returns the tier (`.kernel`)."""
        _capi.check(self._L.ldpc_osd_device_prepare(self._h, device_option(device), int(kernel_variant)), self._L)
        return self.kernel

    @property
    def kernel(self) -> int:
        """Tier of the device form (ldpc_osd_device_kernel): 1 one wave per syndrome, 2 one workgroup per syndrome
        (state in LDS), 3 unlimited (state in a global workspace); 0 = not prepared."""
        return int(self._L.ldpc_osd_device_kernel(self._h)) if self._h else 0

    def postprocess_device(self, syn, bp_err, llr, out=None, stream=None):
        """torch tensors on the prepared device: syn [B][s] u8, bp_err [B][n] u8, llr [B][n] f64, all contiguous
        -> errors [B][n] u8 (`out`; may be `bp_err` itself: in place).  Asynchronous on `stream` (a hipStream_t as
        int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        if out is None:
            out = torch.empty((B, self.n), dtype=torch.uint8, device=bp_err.device)
        _capi.check(self._L.ldpc_osd_postprocess_batch_device(
            self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(bp_err, torch.uint8, (B, self.n)),
            tensor_ptr(llr, torch.float64, (B, self.n)), tensor_ptr(out, torch.uint8, (B, self.n)), stream_ptr(stream, bp_err)), self._L)
        return out


class BeliefPropagationOSDDecoder(AbstractDecoder):
    """`BeliefPropagationOSDDecoder(H, per, max_iters; osd_order=0)` (belief_propagation_osd.jl:26-29).
    osd="host" (default): the ordered-statistics step in host threads; osd="device": in HIP kernels on the BP
    decoder's GPU (`OSDPostProcessor.postprocess_device`), so that `batchdecode_device` never leaves the device."""

    def __init__(self, H, per: float = None, max_iters: int = None, *, osd_order: int = 0, osd: str = "host",
                 bp_decoder=None, osd_method: str = "reference", osd_weights="hamming", **bp_kwargs):
        """bp_decoder: a decoder object to use as `self.bp_decoder` instead of constructing a BeliefPropagationDecoder --
        anything with `decode_batch_host(syn, want_llr=True)`, `decode_batch_device(syn, err, conv, llr, iters)`,
        `.s`, `.n`, `.sparse_H`, `.scratch` and `info().device`, such as a MinSumDecoder.  Its pattern must equal H's
        (ValueError otherwise); `per` and `max_iters` are then IGNORED (the object carries its own priors and iteration
        count) and no other decoder keyword may be given.
        osd_method: "reference" (default), "exhaustive" or "combination_sweep" -- the standard rule, osd="device" only.
        osd_weights, for the standard rule: "hamming" (all ones), "priors" (log((1 - per) / per), or the `channel_llr`
        of the bp_decoder= object) or an array of n channel LLRs."""
        if osd not in ("host", "device"):
            raise ValueError('osd must be "host" or "device"')
        if osd_method not in OSD_METHODS:
            raise ValueError('osd_method must be "reference", "exhaustive" or "combination_sweep"')
        if osd_method != "reference" and osd != "device":
            raise ValueError('osd_method="%s" has a device form only: pass osd="device"' % osd_method)
        if isinstance(osd_weights, str) and osd_weights not in ("hamming", "priors"):
            raise ValueError('osd_weights must be "hamming", "priors" or an array of channel LLRs')
        if osd_method == "reference" and not (isinstance(osd_weights, str) and osd_weights == "hamming"):
            raise ValueError("the reference rule weighs by count: osd_weights needs another osd_method")
        if bp_decoder is not None:
            if bp_kwargs:
                raise TypeError("decoder keywords (%s) have no meaning next to bp_decoder=" % ", ".join(sorted(bp_kwargs)))
            M, D = _pattern_of(H), bp_decoder.sparse_H
            if M.shape != D.shape or not (np.array_equal(M.indptr, D.indptr) and np.array_equal(M.indices, D.indices)):
                raise ValueError("bp_decoder was built on another parity-check matrix than H")
            self.bp_decoder = bp_decoder
        else:
            if per is None or max_iters is None:
                raise TypeError("per and max_iters are required without bp_decoder=")
            # (exact LLRs: OSD orders the bits by reliability, :53-55 -- two that differ beyond the 21st bit must not tie)
            bp_kwargs.setdefault("llr_exact", True)
            self.bp_decoder = BeliefPropagationDecoder(H, per, max_iters, **bp_kwargs)   # :27
        self.H = H                                                                    # :21
        self.osd_order = int(osd_order)                                               # :23
        self.osd_method = osd_method
        if isinstance(osd_weights, str) and osd_weights == "hamming":
            weights = None
        elif isinstance(osd_weights, str):   # "priors"
            if bp_decoder is not None:
                if getattr(bp_decoder, "channel_llr", None) is None:
                    raise ValueError('osd_weights="priors": the bp_decoder= object has no channel_llr')
                weights = np.asarray(bp_decoder.channel_llr, dtype=np.float64)
            else:
                weights = np.full(int(_pattern_of(H).shape[1]), np.log((1.0 - per) / per), dtype=np.float64)
        else:
            weights = osd_weights
        self._osd = OSDPostProcessor(H, osd_order, method=osd_method, weights=weights)
        self.osd = osd
        if osd == "device":
            self._osd.prepare_device(self.bp_decoder.info().device)

    def _postprocess_host_arrays(self, syn_bs, err, llr, nthreads):
        """The OSD step on host arrays: host threads, or (osd="device") the kernel through device copies."""
        if self.osd != "device":
            return self._osd.postprocess(syn_bs, err, llr, nthreads=nthreads)
        import torch

        dev = torch.device("cuda", self.bp_decoder.info().device)
        d_syn = torch.from_numpy(np.ascontiguousarray(syn_bs, dtype=np.uint8)).to(dev)
        d_err = torch.from_numpy(np.ascontiguousarray(err, dtype=np.uint8)).to(dev)
        d_llr = torch.from_numpy(np.ascontiguousarray(llr, dtype=np.float64)).to(dev)
        with torch.cuda.device(dev):
            self._osd.postprocess_device(d_syn, d_err, d_llr, out=d_err)
        return d_err.cpu().numpy()

    def decode_(self, syndrome) -> Tuple[np.ndarray, bool]:
        """`decode!(decoder::BeliefPropagationOSDDecoder, syndrome)` (:49-61): returns
        (error estimate as a Bool vector, whether BP converged)."""
        syn = syndrome_bytes(np.asarray(syndrome).reshape(-1))
        bp = self.bp_decoder
        if syn.size != bp.s:
            raise IndexError(f"syndrome has length {syn.size}, decoder has {bp.s} checks")
        err, conv, llr, _ = bp.decode_batch_host(syn.reshape(1, -1), want_llr=True)        # :51-52
        bp.scratch.err[:] = err[0]
        bp.scratch.log_probabs[:] = llr[0]
        out = self._postprocess_host_arrays(syn.reshape(1, -1), err, llr, 1)               # :53-60
        return out[0].astype(np.bool_), bool(conv[0])

    def batchdecode_(self, syndromes, errors, success=None, nthreads: int = 0):
        """Batch form.  The reference takes the generic per-column loop for BP+OSD
        (abstract_decoder.jl:31-42, test_bposd_decoder.jl:49-57); one BP launch plus one threaded
        OSD pass gives the same columns."""
        syndromes = np.asarray(syndromes)
        B = syndromes.shape[1]
        if success is None:
            success = np.empty(B, dtype=np.bool_)
        assert syndromes.shape[1] == errors.shape[1]
        assert syndromes.shape[1] == len(success)
        bp = self.bp_decoder
        syn_bs = np.ascontiguousarray(syndrome_bytes(syndromes).T)
        err, conv, llr, _ = bp.decode_batch_host(syn_bs, want_llr=True)
        out = self._postprocess_host_arrays(syn_bs, err, llr, nthreads)
        errors[:, :] = out.T
        success[:] = conv.astype(np.bool_)
        if B > 0:
            bp.scratch.err[:] = err[-1]
            bp.scratch.log_probabs[:] = llr[-1]
        return errors, success

    def batchdecode_device(self, syn, nthreads: int = 0):
        """HBM-resident batch (BASELINE config 5 shape): `syn` is a [B][s] uint8 torch tensor on the
        GPU.  BP runs on the device; only the syndromes that still need OSD travel to the host:
        with osd_order = 0 a converged syndrome is returned unchanged by the reference's shortcut
        (belief_propagation_osd.jl:66-74: zero residual), so its OSD call is skipped; with
        osd_order > 0 every syndrome is post-processed, like the reference.  The standard rule (osd_method=) has the
        shortcut at every order, so only the unconverged syndromes are sent at every order.
        Returns (errors [B][n] uint8 tensor, converged [B] uint8 tensor, number sent to OSD).
        With osd="device" nothing of the payload leaves the GPU: the same two passes for osd_order = 0, the OSD
        kernel on the compacted unconverged rows and an index scatter; for osd_order > 0 one BP pass with LLRs and
        the OSD kernel in place on the whole batch."""
        import torch

        bp = self.bp_decoder
        B = int(syn.shape[0])
        dev = syn.device
        if self.osd == "device":
            return self._batchdecode_device_resident(syn)
        err = torch.empty((B, bp.n), dtype=torch.uint8, device=dev)
        conv = torch.empty(B, dtype=torch.uint8, device=dev)
        if self.osd_order == 0 and getattr(self, "_osd_frac", 0.0) <= 0.2:
            # Two passes: BP without LLRs for everybody (no 8n-byte LLR row per syndrome: 1.9 instead of
            # 2.4 ms per 2^20 BB-72 syndromes), then the few unconverged ones once more WITH LLRs -- the
            # decoder is deterministic per syndrome, so their hard decisions come out the same and the
            # LLRs are the ones the one-pass run would have written.  If a batch turns out to need OSD for
            # more than a fifth of its syndromes, later batches go back to one pass.
            bp.decode_batch_device(syn, err, conv, None, None)
            idx = torch.nonzero(conv == 0, as_tuple=False).flatten()
            k = int(idx.numel())
            self._osd_frac = k / max(B, 1)
            if k:
                sub = syn[idx].contiguous()
                e2 = torch.empty((k, bp.n), dtype=torch.uint8, device=dev)
                c2 = torch.empty(k, dtype=torch.uint8, device=dev)
                l2 = torch.empty((k, bp.n), dtype=torch.float64, device=dev)
                bp.decode_batch_device(sub, e2, c2, l2, None)
                out = self._osd.postprocess(sub.cpu().numpy(), e2.cpu().numpy(), l2.cpu().numpy(), nthreads=nthreads)
                err[idx] = torch.from_numpy(out).to(dev)
            return err, conv, k
        llr = torch.empty((B, bp.n), dtype=torch.float64, device=dev)
        bp.decode_batch_device(syn, err, conv, llr, None)
        if self.osd_order == 0:
            idx = torch.nonzero(conv == 0, as_tuple=False).flatten()
        else:
            idx = torch.arange(B, device=dev)
        k = int(idx.numel())
        self._osd_frac = k / max(B, 1) if self.osd_order == 0 else 1.0
        if k:
            out = self._osd.postprocess(syn[idx].cpu().numpy(), err[idx].cpu().numpy(), llr[idx].cpu().numpy(),
                                        nthreads=nthreads)
            err[idx] = torch.from_numpy(out).to(dev)
        return err, conv, k

    def _batchdecode_device_resident(self, syn):
        import torch

        bp = self.bp_decoder
        B = int(syn.shape[0])
        dev = syn.device
        err = torch.empty((B, bp.n), dtype=torch.uint8, device=dev)
        conv = torch.empty(B, dtype=torch.uint8, device=dev)
        if self.osd_order > 0 and self.osd_method == "reference":
            llr = torch.empty((B, bp.n), dtype=torch.float64, device=dev)
            bp.decode_batch_device(syn, err, conv, llr, None)
            if B:
                self._osd.postprocess_device(syn, err, llr, out=err)
            return err, conv, B
        # order 0, and the standard rule at every order (its step 1 returns a converged estimate unchanged)
        if getattr(self, "_osd_frac", 0.0) <= 0.2:
            # two passes, as on the host path: no 8n-byte LLR row for the syndromes BP converges on
            bp.decode_batch_device(syn, err, conv, None, None)
            idx = torch.nonzero(conv == 0, as_tuple=False).flatten()   # (its size is the one scalar the host reads)
            k = int(idx.numel())
            self._osd_frac = k / max(B, 1)
            if k:
                sub = syn[idx].contiguous()
                e2 = torch.empty((k, bp.n), dtype=torch.uint8, device=dev)
                c2 = torch.empty(k, dtype=torch.uint8, device=dev)
                l2 = torch.empty((k, bp.n), dtype=torch.float64, device=dev)
                bp.decode_batch_device(sub, e2, c2, l2, None)
                self._osd.postprocess_device(sub, e2, l2, out=e2)
                err[idx] = e2
            return err, conv, k
        # many unconverged: one pass with LLRs; the kernel returns the BP estimate of a converged syndrome unchanged
        # (zero residual, :72-74), so it runs in place on the whole batch
        llr = torch.empty((B, bp.n), dtype=torch.float64, device=dev)
        bp.decode_batch_device(syn, err, conv, llr, None)
        k = int((conv == 0).sum())
        self._osd_frac = k / max(B, 1)
        if k:
            self._osd.postprocess_device(syn, err, llr, out=err)
        return err, conv, k
