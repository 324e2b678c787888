"""BP-OTS decoder: host mirror of `BPOTSDecoder` (src/decoders/bpots_decoder.jl:39-115) over the
ldpc_bpots_* entry points; decode!/batchdecode! as in :225-340 and abstract_decoder.jl:31-48."""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _capi, _host
from ._host import Handle, _pattern_of, csc_arrays, device_option, host_batch, stream_ptr, tensor_ptr
from .decoder import AbstractDecoder


BPOTSPlan = namedtuple("BPOTSPlan", "kernel S lds_bytes budget_kib DC DV")
BPOTSLaunch = namedtuple("BPOTSLaunch", "path groups grid chunk per_cu")


def bpots_plan(s, n, nnz, max_cdeg, max_bdeg, force_node=0, experiments=False) -> BPOTSPlan:
    """What ldpc_bpots_create would choose for such a graph (ldpc_debug_bpots_plan; no device needed): the kernel (2, 3, 5),
    S syndromes per workgroup (0 outside the LDS kernel), its dynamic LDS bytes, the budget in KiB (76, 156; 0 outside the
    LDS kernel) and the register buckets DC, DV (0 for kernel 5)."""
    L = _capi.lib(experiments)
    k, logS, b, dc, dv = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    nbytes = ctypes.c_int64()
    _capi.check(L.ldpc_debug_bpots_plan(int(s), int(n), int(nnz), int(max_cdeg), int(max_bdeg), int(force_node), ctypes.byref(k),
                                        ctypes.byref(logS), ctypes.byref(nbytes), ctypes.byref(b), ctypes.byref(dc), ctypes.byref(dv)), L)
    return BPOTSPlan(k.value, 1 << logS.value if logS.value >= 0 else 0, nbytes.value, b.value, dc.value, dv.value)


def bpots_plan_of(H, force_node=0, experiments=False) -> BPOTSPlan:
    """bpots_plan of a parity-check matrix (anything BPOTSDecoder takes)."""
    M = _pattern_of(H)
    cdeg, bdeg = np.diff(M.tocsr().indptr), np.diff(M.tocsc().indptr)
    return bpots_plan(M.shape[0], M.shape[1], M.nnz, int(cdeg.max(initial=0)), int(bdeg.max(initial=0)), force_node, experiments)


class BPOTSDecoder(AbstractDecoder, Handle):
    """`BPOTSDecoder(H, per::Float64, max_iters::Int; T::Int=9, C::Float64=2.0)`.  `decode_` returns best_decisions as an
    Int vector; there is no host scratch."""

    _destroy = "ldpc_bpots_destroy"
    _scratch_keeps = ()
    decode_, batchdecode_ = _host.decode_, _host.batchdecode_

    def __init__(self, H, per: float, max_iters: int, *, T: int = 9, C: float = 2.0, device=None, experiments=None):
        if not isinstance(per, float):
            raise TypeError("per must be a Float64")
        M = _pattern_of(H)
        self.per, self.max_iters, self.T, self.C = float(per), int(max_iters), int(T), float(C)
        self.s, self.n = int(M.shape[0]), int(M.shape[1])
        self.sparse_H = M
        colptr, rowval = csc_arrays(M)
        L = _capi.lib_for(experiments)
        self._create(L, L.ldpc_bpots_create, self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                     self.per, self.max_iters, self.T, self.C, device_option(device))

    @property
    def kernel(self) -> int:
        """2 = LDS-resident kernel, 3 = node-parallel kernel with the messages in a global slot (ldpc_bpots_kernel)."""
        return int(self._L.ldpc_bpots_kernel(self._h))

    def last_launch(self) -> BPOTSLaunch:
        """How the most recent decode was launched (ldpc_debug_bpots_last_launch): path 0 none / 1 latency / 2 queue,
        groups, workgroups, groups per queue ticket, workgroups per CU by the occupancy query (LDS kernel only)."""
        path, grid, chunk, per_cu, groups = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        _capi.check(self._L.ldpc_debug_bpots_last_launch(self._h, ctypes.byref(path), ctypes.byref(groups), ctypes.byref(grid),
                                                         ctypes.byref(chunk), ctypes.byref(per_cu)), self._L)
        return BPOTSLaunch(path.value, groups.value, grid.value, chunk.value, per_cu.value)

    def decode_batch_host(self, syn_bs):
        """syn [B][s] uint8 -> (errors [B][n] u8 = best_decisions, converged [B] u8, iters [B] i32)."""
        syn, B, err, conv, _, its = host_batch(syn_bs, self.s, self.n)
        _capi.check(self._L.ldpc_bpots_decode_batch(self._h, B, syn.ctypes.data, err.ctypes.data,
                                                    conv.ctypes.data, its.ctypes.data), self._L)
        return err, conv, its

    def decode_batch_device(self, syn, err, conv, iters=None, stream=None) -> None:
        """HBM-resident batch (ldpc_bpots_decode_batch_device): torch tensors on the decoder's GPU, syn [B][s] u8,
        err [B][n] u8, conv [B] u8, iters [B] i32 | None, all contiguous.  Asynchronous on `stream` (a hipStream_t as
        int; default = torch's current stream)."""
        import torch

        B = int(syn.shape[0])
        _capi.check(self._L.ldpc_bpots_decode_batch_device(
            self._h, B, tensor_ptr(syn, torch.uint8, (B, self.s)), tensor_ptr(err, torch.uint8, (B, self.n)),
            tensor_ptr(conv, torch.uint8, B), tensor_ptr(iters, torch.int32, B, optional=True), stream_ptr(stream, syn)), self._L)
