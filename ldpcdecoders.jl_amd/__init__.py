"""MI355X-native belief-propagation LDPC decoder behind LDPCDecoders.jl's BP API.

The directory is called ``ldpcdecoders.jl_amd``; because of the dot it is
imported through the loader module ``ldpcdecoders_jl_amd`` at the repo root::

    import ldpcdecoders_jl_amd as ldpc
    dec = ldpc.BeliefPropagationDecoder(H, 0.01, 50)
    guess, ok = ldpc.decode_(dec, syndrome)

Exports follow src/LDPCDecoders.jl:12-18 for the hot path (``!`` -> ``_``).
"""
from . import _capi, codes  # noqa: F401
from ._capi import LdpcError, build  # noqa: F401
from .bitmatrix import BitMatrix  # noqa: F401
from .codes import load_pcm, parity_check_matrix, save_pcm  # noqa: F401
from .decoder import (  # noqa: F401
    AbstractDecoder,
    BeliefPropagationDecoder,
    BeliefPropagationScratchSpace,
    batchdecode_,
    decode_,
    reset_,
    syndrome_bytes,
)

from .osd import BeliefPropagationOSDDecoder, OSDPostProcessor  # noqa: F401,E402
from .bpots import BPOTSDecoder  # noqa: F401,E402
from .bitflip import BitFlipDecoder, BitFlipScratchSpace  # noqa: F401,E402
from .minsum import MinSumDecoder, MinSumScratchSpace  # noqa: F401,E402
from .relay import RelayMinSumDecoder  # noqa: F401,E402
from .decim import DecimatedMinSumDecoder  # noqa: F401,E402
from .trials import TrialResult, Trials, run_trials  # noqa: F401,E402
from .css_trials import CSSTrialResult, CSSTrials, conditional_probs, run_css_joint_trials, run_css_trials  # noqa: F401,E402
from .pauli import PauliMinSumDecoder  # noqa: F401,E402
from .pauli_relay import PauliRelayMinSumDecoder  # noqa: F401,E402
from .stabilizer import StabilizerMinSumDecoder, run_stabilizer_trials  # noqa: F401,E402
from .dem import DetectorErrorModel, phenomenological, run_dem_trials  # noqa: F401,E402
from .windows import SlidingWindowDecoder, WindowPlan, WindowStep, phenomenological_layers, window_plan  # noqa: F401,E402

__all__ = [
    "BeliefPropagationOSDDecoder", "OSDPostProcessor", "BPOTSDecoder", "BitFlipDecoder", "BitFlipScratchSpace",
    "decode_", "batchdecode_", "reset_", "AbstractDecoder", "BeliefPropagationDecoder",
    "BeliefPropagationScratchSpace", "parity_check_matrix", "save_pcm", "load_pcm",
    "LdpcError", "build", "codes", "syndrome_bytes", "BitMatrix",
    "MinSumDecoder", "MinSumScratchSpace", "RelayMinSumDecoder", "DecimatedMinSumDecoder",
    "Trials", "TrialResult", "run_trials",
    "CSSTrials", "CSSTrialResult", "run_css_trials", "run_css_joint_trials", "conditional_probs", "PauliMinSumDecoder",
    "PauliRelayMinSumDecoder", "StabilizerMinSumDecoder", "run_stabilizer_trials",
    "DetectorErrorModel", "phenomenological", "run_dem_trials",
    "SlidingWindowDecoder", "WindowPlan", "WindowStep", "phenomenological_layers", "window_plan",
]
