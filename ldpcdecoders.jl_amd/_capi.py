"""ctypes binding of libldpc_mi355x.so (include/ldpc_mi355x.h).

This is the same C ABI the Julia `ccall` shim binds.  There is
no fallback of any kind: a missing library or a missing gfx950 device raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# LDPC_MI355X_LIB selects another build of the same library (tuning experiments, installed copies)
LIB_PATH = os.environ.get("LDPC_MI355X_LIB") or os.path.join(CSRC, "libldpc_mi355x.so")
# The experiments build (-DLDPC_EXPERIMENTS): the same code plus the environment knobs and the fault injection that
# tests and tools use to force a code path.  The product library above reads no environment variable.
EXP_LIB_PATH = os.environ.get("LDPC_MI355X_EXP_LIB") or os.path.join(CSRC, "libldpc_mi355x_exp.so")

LDPC_OK = 0
STATUS_NAMES = {
    0: "LDPC_OK",
    1: "LDPC_ERR_INVALID_ARGUMENT",
    2: "LDPC_ERR_NO_DEVICE",
    3: "LDPC_ERR_HIP",
    4: "LDPC_ERR_OUT_OF_MEMORY",
    5: "LDPC_ERR_UNSUPPORTED",
}

MULTI_MAX_DEVICES = 16
EXCHANGE_AUTO, EXCHANGE_COPY, EXCHANGE_RCCL, EXCHANGE_NONE = 0, 1, 2, 3


class LdpcError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status
        self.message = message


class BPInfo(ctypes.Structure):
    _fields_ = [
        ("s", ctypes.c_int64), ("n", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("max_iters", ctypes.c_int64), ("per", ctypes.c_double),
        ("max_check_degree", ctypes.c_int32), ("max_bit_degree", ctypes.c_int32),
        ("device", ctypes.c_int32), ("tile_syndromes", ctypes.c_int32),
        ("waves_per_tile", ctypes.c_int32), ("resident_tiles", ctypes.c_int32),
        ("workspace_bytes", ctypes.c_int64),
        ("last_kernel", ctypes.c_int32), ("last_team_size", ctypes.c_int32),
        ("last_lds_rows", ctypes.c_int32), ("last_rows_on_chip", ctypes.c_int32), ("reserved_info", ctypes.c_int32 * 2),
    ]


class BPMultiInfo(ctypes.Structure):
    _fields_ = [
        ("ndev", ctypes.c_int32), ("exchange", ctypes.c_int32), ("devices", ctypes.c_int32 * MULTI_MAX_DEVICES),
        ("scatter_ms", ctypes.c_double), ("root_decode_ms", ctypes.c_double), ("gather_ms", ctypes.c_double),
        ("decode_ms_max", ctypes.c_double),
        ("scatter_bytes_per_peer", ctypes.c_int64), ("gather_bytes_per_peer", ctypes.c_int64),
    ]


class BPOptions(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32), ("waves_per_tile", ctypes.c_int32),
        ("resident_tiles", ctypes.c_int32), ("kernel_variant", ctypes.c_int32),
        ("defer_threshold", ctypes.c_int32), ("llr_exact", ctypes.c_int32), ("reserved", ctypes.c_int32 * 10),
    ]


BF_TIE_RANDOM, BF_TIE_FIRST, BF_TIE_LAST = 0, 1, 2


class BitFlipOptions(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32), ("tie_break", ctypes.c_int32), ("seed", ctypes.c_uint64),
        ("kernel_variant", ctypes.c_int32), ("reserved", ctypes.c_int32 * 11),
    ]


class MinSumOptions(ctypes.Structure):
    """ldpc_minsum_options: alpha = 0 / clip = 0 select the defaults (0.75, 1e6); schedule 0 = flooding, 1 = layered."""
    _fields_ = [
        ("device", ctypes.c_int32), ("alpha", ctypes.c_float), ("clip", ctypes.c_float),
        ("kernel_variant", ctypes.c_int32), ("schedule", ctypes.c_int32), ("reserved", ctypes.c_int32 * 11),
    ]


class RelayOptions(ctypes.Structure):
    """ldpc_relay_options: alpha = 0 / clip = 0 / stop_after = 0 select the defaults (0.75, 1e6, 1)."""
    _fields_ = [
        ("device", ctypes.c_int32), ("alpha", ctypes.c_float), ("clip", ctypes.c_float),
        ("kernel_variant", ctypes.c_int32), ("stop_after", ctypes.c_int32), ("reserved", ctypes.c_int32 * 11),
    ]


class DecimOptions(ctypes.Structure):
    """ldpc_decim_options: alpha = 0 / clip = 0 select the defaults (0.75, 1e6)."""
    _fields_ = [
        ("device", ctypes.c_int32), ("alpha", ctypes.c_float), ("clip", ctypes.c_float),
        ("kernel_variant", ctypes.c_int32), ("reserved", ctypes.c_int32 * 12),
    ]


class PauliMinSumOptions(ctypes.Structure):
    """ldpc_pauli_minsum_options: alpha = 0 / clip = 0 select the defaults (0.75, 1e6)."""
    _fields_ = [
        ("device", ctypes.c_int32), ("alpha", ctypes.c_float), ("clip", ctypes.c_float),
        ("kernel_variant", ctypes.c_int32), ("reserved", ctypes.c_int32 * 12),
    ]


class PauliRelayOptions(ctypes.Structure):
    """ldpc_pauli_relay_options: alpha = 0 / clip = 0 / stop_after = 0 select the defaults (0.75, 1e6, 1)."""
    _fields_ = [
        ("device", ctypes.c_int32), ("alpha", ctypes.c_float), ("clip", ctypes.c_float),
        ("kernel_variant", ctypes.c_int32), ("stop_after", ctypes.c_int32), ("reserved", ctypes.c_int32 * 11),
    ]


class StabMinSumOptions(ctypes.Structure):
    """ldpc_stab_minsum_options: alpha = 0 / clip = 0 select the defaults (0.75, 1e6)."""
    _fields_ = [
        ("device", ctypes.c_int32), ("alpha", ctypes.c_float), ("clip", ctypes.c_float),
        ("kernel_variant", ctypes.c_int32), ("reserved", ctypes.c_int32 * 12),
    ]


class TrialsOptions(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("kernel_variant", ctypes.c_int32), ("reserved", ctypes.c_int32 * 14)]


class CSSPattern(ctypes.Structure):
    """ldpc_css_pattern: a zero-based CSC pattern of `rows` rows."""
    _fields_ = [("rows", ctypes.c_int64), ("nnz", ctypes.c_int64), ("colptr", ctypes.c_void_p), ("rowval", ctypes.c_void_p)]


class CSSTrialsOptions(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("kernel_variant", ctypes.c_int32), ("reserved", ctypes.c_int32 * 14)]


class WindowsOptions(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("reserved", ctypes.c_int32 * 15)]


# The prototypes, name -> (restype, argtypes): the one list of what the library exports.  ldpc_status is an int32_t; a
# handle and every array is a void pointer, a structure or a fixed-size array goes by a typed pointer.
vp, i32, i64, u64, f64, cstr, P = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double,
                                   ctypes.c_char_p, ctypes.POINTER)
# every function include/ldpc_mi355x.h declares
API = {
    "ldpc_abi_version": (i32, []),
    "ldpc_build_target": (cstr, []),
    "ldpc_last_error": (cstr, []),
    "ldpc_device_count": (i32, []),
    "ldpc_trim_memory": (i32, []),
    "ldpc_set_wait_limit_ms": (i32, [i64]),
    "ldpc_get_wait_limit_ms": (i64, []),
    "ldpc_bp_create": (i32, [i64, i64, i64, vp, vp, f64, i64, P(BPOptions), P(vp)]),
    "ldpc_bp_destroy": (i32, [vp]),
    "ldpc_bp_get_info": (i32, [vp, P(BPInfo)]),
    "ldpc_bp_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_bp_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_bp_decode_batch_bits": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, vp]),
    "ldpc_bp_decode_batch_bits_device": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp]),
    "ldpc_bp_last_status": (i32, [vp]),
    "ldpc_bp_last_timing": (i32, [vp, P(f64), P(f64), P(i64)]),
    "ldpc_bp_call_timing": (i32, [vp, i32, P(f64), P(f64), P(i64)]),
    "ldpc_bp_call_phase_ticks": (i32, [vp, i32, P(u64 * 3)]),
    "ldpc_bp_create_multi": (i32, [i32, P(i32), i32, i64, i64, i64, vp, vp, f64, i64, P(BPOptions), P(vp)]),
    "ldpc_bp_destroy_multi": (i32, [vp]),
    "ldpc_bp_multi_handle": (vp, [vp, i32]),
    "ldpc_bp_decode_batch_multi": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_bp_decode_batch_multi_bits": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, vp]),
    "ldpc_bp_decode_batch_multi_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_bp_multi_last_status": (i32, [vp]),
    "ldpc_bp_multi_get_info": (i32, [vp, P(BPMultiInfo)]),
    "ldpc_osd_create": (i32, [i64, i64, i64, vp, vp, i64, P(vp)]),
    "ldpc_osd_destroy": (i32, [vp]),
    "ldpc_osd_postprocess_batch": (i32, [vp, i64, vp, vp, vp, vp, i32]),
    "ldpc_osd_device_prepare": (i32, [vp, i32, i32]),
    "ldpc_osd_device_kernel": (i32, [vp]),
    "ldpc_osd_postprocess_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_bpots_create": (i32, [i64, i64, i64, vp, vp, f64, i64, i64, f64, i32, P(vp)]),
    "ldpc_bpots_destroy": (i32, [vp]),
    "ldpc_bpots_kernel": (i32, [vp]),
    "ldpc_bpots_decode_batch": (i32, [vp, i64, vp, vp, vp, vp]),
    "ldpc_bpots_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_bitflip_create": (i32, [i64, i64, i64, vp, vp, f64, i64, P(BitFlipOptions), P(vp)]),
    "ldpc_bitflip_destroy": (i32, [vp]),
    "ldpc_bitflip_kernel": (i32, [vp]),
    "ldpc_bitflip_decode_batch": (i32, [vp, i64, i64, vp, vp, vp, vp, vp]),
    "ldpc_bitflip_decode_batch_device": (i32, [vp, i64, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_minsum_create": (i32, [i64, i64, i64, vp, vp, vp, i64, P(MinSumOptions), P(vp)]),
    "ldpc_minsum_destroy": (i32, [vp]),
    "ldpc_minsum_kernel": (i32, [vp]),
    "ldpc_minsum_tile_syndromes": (i32, [vp]),
    "ldpc_minsum_last_grid": (i32, [vp]),
    "ldpc_minsum_layers": (i32, [vp]),
    "ldpc_minsum_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_minsum_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_minsum_priors_kernel": (i32, [vp]),
    "ldpc_minsum_priors_tile_syndromes": (i32, [vp]),
    "ldpc_minsum_decode_batch_priors": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_minsum_decode_batch_priors_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_minsum_set_conditional_priors": (i32, [vp, vp, vp]),
    "ldpc_minsum_decode_batch_given": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_minsum_decode_batch_given_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_relay_create": (i32, [i64, i64, i64, vp, vp, vp, i64, vp, vp, P(RelayOptions), P(vp)]),
    "ldpc_relay_destroy": (i32, [vp]),
    "ldpc_relay_kernel": (i32, [vp]),
    "ldpc_relay_tile_syndromes": (i32, [vp]),
    "ldpc_relay_last_grid": (i32, [vp]),
    "ldpc_relay_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_relay_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_pauli_minsum_create": (i32, [i64, P(CSSPattern), P(CSSPattern), vp, vp, vp, i64, P(PauliMinSumOptions), P(vp)]),
    "ldpc_pauli_minsum_destroy": (i32, [vp]),
    "ldpc_pauli_minsum_kernel": (i32, [vp]),
    "ldpc_pauli_minsum_tile_syndromes": (i32, [vp]),
    "ldpc_pauli_minsum_last_grid": (i32, [vp]),
    "ldpc_pauli_minsum_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_pauli_minsum_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_trials_create": (i32, [i64, i64, i64, vp, vp, i64, i64, vp, vp, P(TrialsOptions), P(vp)]),
    "ldpc_trials_destroy": (i32, [vp]),
    "ldpc_trials_kernel": (i32, [vp]),
    "ldpc_trials_sample_device": (i32, [vp, i64, i64, f64, u64, vp, vp, vp]),
    "ldpc_trials_syndromes_device": (i32, [vp, i64, vp, vp, vp]),
    "ldpc_trials_score_device": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_trials_sample": (i32, [vp, i64, i64, f64, u64, vp, vp]),
    "ldpc_trials_score": (i32, [vp, i64, vp, vp, vp, vp]),
    "ldpc_trials_set_rates": (i32, [vp, i64, vp]),
    "ldpc_trials_sample_rates_device": (i32, [vp, i64, i64, u64, vp, vp, vp]),
    "ldpc_trials_sample_rates": (i32, [vp, i64, i64, u64, vp, vp]),
    "ldpc_css_trials_create": (i32, [i64, P(CSSPattern), P(CSSPattern), P(CSSPattern), P(CSSPattern), P(CSSTrialsOptions), P(vp)]),
    "ldpc_css_trials_destroy": (i32, [vp]),
    "ldpc_css_trials_kernel": (i32, [vp]),
    "ldpc_css_trials_sample_device": (i32, [vp, i64, i64, f64, f64, f64, u64, vp, vp, vp, vp, vp]),
    "ldpc_css_trials_syndromes_device": (i32, [vp, i64, vp, vp, vp, vp, vp]),
    "ldpc_css_trials_score_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_css_trials_sample": (i32, [vp, i64, i64, f64, f64, f64, u64, vp, vp, vp, vp]),
    "ldpc_css_trials_score": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_windows_create": (i32, [i64, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, P(WindowsOptions), P(vp)]),
    "ldpc_windows_destroy": (i32, [vp]),
    "ldpc_windows_count": (i64, [vp]),
    "ldpc_windows_gather_device": (i32, [vp, i64, i64, vp, vp, vp]),
    "ldpc_windows_commit_device": (i32, [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp]),
}
# ... and include/ldpc_mi355x_debug.h (test hooks, not part of the boundary)
DEBUG_API = {
    "ldpc_debug_team_rows": (i32, [i64, i64, vp, vp, i32, i32, i32, P(i32 * 2), P(i32 * 5), vp, vp, vp, vp]),
    "ldpc_debug_team_plan": (i32, [i64, i64, i64, i32, i32, P(i32 * 6)]),
    "ldpc_debug_div_check": (i32, [i64, vp, vp, vp, vp]),
    "ldpc_debug_process_state": (vp, []),
    "ldpc_debug_adopt_process_state": (i32, [vp]),
    "ldpc_debug_team_irr": (i32, [i64, i64, vp, vp, i32, i32, i32, P(i32 * 2), vp, vp, vp, vp, vp]),
    "ldpc_debug_llr_check": (i32, [i64, vp, vp, vp]),
    "ldpc_debug_tile_plan": (i32, [i64, i64, i64, i32, i32, P(i32), P(i32), P(i64)]),
    "ldpc_debug_layer_plan": (i32, [i64, i64, vp, vp, vp, P(i32)]),
    "ldpc_debug_priors_tile_plan": (i32, [i64, i64, i64, i32, i32, P(i32), P(i32), P(i64)]),
    "ldpc_debug_pauli_tile_plan": (i32, [i64, i64, i64, i32, P(i32), P(i32), P(i64)]),
    "ldpc_debug_bpots_plan": (i32, [i64, i64, i64, i32, i32, i32, P(i32), P(i32), P(i64), P(i32), P(i32), P(i32)]),
    "ldpc_debug_bpots_last_launch": (i32, [vp, P(i32), P(i64), P(i32), P(i32), P(i32)]),
}
# The guided-decimation min-sum decoder: include/ldpc_mi355x_decim.h (a part of ldpc_mi355x.h) and its test hook,
# include/ldpc_mi355x_decim_debug.h (a part of ldpc_mi355x_debug.h).  The two tables above stay what the two headers
# themselves declare; these follow the same conventions and are bound with them.
DECIM_API = {
    "ldpc_decim_create": (i32, [i64, i64, i64, vp, vp, vp, i64, i64, P(DecimOptions), P(vp)]),
    "ldpc_decim_destroy": (i32, [vp]),
    "ldpc_decim_kernel": (i32, [vp]),
    "ldpc_decim_tile_syndromes": (i32, [vp]),
    "ldpc_decim_last_grid": (i32, [vp]),
    "ldpc_decim_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_decim_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
}
DECIM_DEBUG_API = {
    "ldpc_debug_decim_tile_plan": (i32, [i64, i64, i64, i32, P(i32), P(i32), P(i64)]),
}
# The standard rule of the OSD step: include/ldpc_mi355x_osd_search.h (a part of ldpc_mi355x.h), bound the same way.
OSD_SEARCH_API = {
    "ldpc_osd_set_search": (i32, [vp, i32, i64, i64, vp]),
    "ldpc_osd_search_method": (i32, [vp]),
    "ldpc_osd_search_weight": (i64, [vp, i64]),
}
# The Pauli relay min-sum decoder: include/ldpc_mi355x_pauli_relay.h (a part of ldpc_mi355x.h) and its test hook,
# include/ldpc_mi355x_pauli_relay_debug.h (a part of ldpc_mi355x_debug.h), bound the same way.
PAULI_RELAY_API = {
    "ldpc_pauli_relay_create": (i32, [i64, P(CSSPattern), P(CSSPattern), vp, vp, vp, i64, vp, vp, P(PauliRelayOptions), P(vp)]),
    "ldpc_pauli_relay_destroy": (i32, [vp]),
    "ldpc_pauli_relay_kernel": (i32, [vp]),
    "ldpc_pauli_relay_tile_syndromes": (i32, [vp]),
    "ldpc_pauli_relay_last_grid": (i32, [vp]),
    "ldpc_pauli_relay_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "ldpc_pauli_relay_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
PAULI_RELAY_DEBUG_API = {
    "ldpc_debug_pauli_relay_tile_plan": (i32, [i64, i64, i64, i32, P(i32), P(i32), P(i64)]),
}
# The stabilizer (non-CSS) min-sum decoder: include/ldpc_mi355x_stab.h (a part of ldpc_mi355x.h) and its test hook,
# include/ldpc_mi355x_stab_debug.h (a part of ldpc_mi355x_debug.h), bound the same way.
STAB_API = {
    "ldpc_stab_minsum_create": (i32, [i64, P(CSSPattern), P(CSSPattern), vp, vp, vp, i64, P(StabMinSumOptions), P(vp)]),
    "ldpc_stab_minsum_destroy": (i32, [vp]),
    "ldpc_stab_minsum_kernel": (i32, [vp]),
    "ldpc_stab_minsum_tile_syndromes": (i32, [vp]),
    "ldpc_stab_minsum_last_grid": (i32, [vp]),
    "ldpc_stab_minsum_decode_batch": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "ldpc_stab_minsum_decode_batch_device": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
}
STAB_DEBUG_API = {
    "ldpc_debug_stab_tile_plan": (i32, [i64, i64, i64, i32, P(i32), P(i32), P(i64)]),
}
EXPORTED_SYMBOLS = tuple(API)
DEBUG_SYMBOLS = tuple(DEBUG_API)
DECIM_SYMBOLS = tuple(DECIM_API)
DECIM_DEBUG_SYMBOLS = tuple(DECIM_DEBUG_API)
OSD_SEARCH_SYMBOLS = tuple(OSD_SEARCH_API)
PAULI_RELAY_SYMBOLS = tuple(PAULI_RELAY_API)
PAULI_RELAY_DEBUG_SYMBOLS = tuple(PAULI_RELAY_DEBUG_API)
STAB_SYMBOLS = tuple(STAB_API)
STAB_DEBUG_SYMBOLS = tuple(STAB_DEBUG_API)


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU).  make decides what is stale: its
    source list is the real one.  `force` asked for the make run that every call now does."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "all"])
    return LIB_PATH


_LIBS = {}


def _one_hip_runtime() -> None:
    """Keep ONE HIP runtime in the process.  PyTorch-ROCm bundles its own libamdhip64.so.7;
    the library links against the same SONAME, so whichever copy is mapped first serves both.
    When torch is installed it must be that copy, or torch tensors / streams handed to
    ldpc_bp_decode_batch_device would belong to a different runtime instance.  Without torch
    (plain ctypes or the Julia shim) the system ROCm runtime is used."""
    if os.environ.get("LDPC_MI355X_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib(experiments: bool = False) -> ctypes.CDLL:
    """Load the HIP library; raises (never falls back) if it is not built.  experiments=True: the build with the
    environment knobs and the fault injection (tests, tools); both builds may live in one process."""
    if experiments in _LIBS:
        return _LIBS[experiments]
    path = EXP_LIB_PATH if experiments else LIB_PATH
    if not os.path.exists(path):
        raise LdpcError(2, f"{path} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C ldpcdecoders.jl_amd/csrc`. There is no CPU fallback.")
    _one_hip_runtime()
    L = ctypes.CDLL(path)
    for group in (API, DEBUG_API, DECIM_API, DECIM_DEBUG_API, OSD_SEARCH_API, PAULI_RELAY_API, PAULI_RELAY_DEBUG_API,
                  STAB_API, STAB_DEBUG_API):
        for name, (restype, argtypes) in group.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    # both builds in one process: the one loaded second orders its team grids through the first one's per-device events,
    # so that no two team grids of the process share a device (include/ldpc_mi355x_debug.h)
    other = _LIBS.get(not experiments)
    if other is not None and os.path.realpath(path) != os.path.realpath(EXP_LIB_PATH if not experiments else LIB_PATH):
        check(L.ldpc_debug_adopt_process_state(other.ldpc_debug_process_state()), L)
    _LIBS[experiments] = L
    return L


def knobs_in_env() -> bool:
    """Is any of the library's experiment knobs (LDPC_TEAM_*, LDPC_DEFER_*, ... DESIGN.md "Environment knobs") set?"""
    return any(k.startswith("LDPC_") and not k.startswith("LDPC_MI355X_") for k in os.environ)


def lib_for(experiments=None) -> ctypes.CDLL:
    """The library a new decoder binds: the product build, unless the caller asks for the experiments build or has
    set one of its knobs in the environment (only that build reads them)."""
    return lib(knobs_in_env() if experiments is None else bool(experiments))


def check(status: int, L: ctypes.CDLL = None) -> None:
    if status != LDPC_OK:
        raise LdpcError(status, (L or lib()).ldpc_last_error().decode("utf-8", "replace"))
