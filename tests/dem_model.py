"""CPU model of the per-bit sample step: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it and nothing
here calls the library.  A plain numpy restatement of the per-bit rule of include/ldpc_mi355x.h (the ldpc_trials_*
section), with k_i, r_ij and mix those of tests/trials_model.py:

    t_j         = (uint64)(rates[j] * 2^64)                        for rates[j] < 1
    error(i, j) = rates[j] >= 1 ? 1 : (r_ij < t_j)                 (uint64 arithmetic)
"""
import numpy as np

from trials_model import GOLDEN, mix, mix_array


def thresholds(rates) -> np.ndarray:
    """t_j as uint64 where rates[j] < 1 (the product is a power-of-two scaling, int() truncates); 0 elsewhere."""
    r = np.asarray(rates, dtype=np.float64).reshape(-1)
    if r.size and not np.all((r >= 0.0) & (r <= 1.0)):   # (False for NaN as well)
        raise ValueError("a rate outside [0, 1]")
    return np.array([int(float(x) * 18446744073709551616.0) if x < 1.0 else 0 for x in r], dtype=np.uint64)


def sample(rates, batch: int, seed: int = 0, column0: int = 0) -> np.ndarray:
    """errors [batch][n] uint8, bit j drawn at rates[j]."""
    r = np.asarray(rates, dtype=np.float64).reshape(-1)
    t = thresholds(r)
    keys = np.array([mix(seed + GOLDEN * (column0 + i + 1)) for i in range(batch)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        draw = mix_array(keys[:, None] + np.arange(r.size, dtype=np.uint64)[None, :])
    return ((draw < t[None, :]) | (r >= 1.0)[None, :]).astype(np.uint8)
