"""CPU model of the Monte-Carlo trial steps: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it and
nothing here calls the library.  A plain numpy restatement of the three rules of include/ldpc_mi355x.h:

    sample     k_i = mix(seed + GOLDEN * (column0 + i + 1)), r_ij = mix(k_i + j), t = (uint64)(per * 2^64),
               error(i, j) = per >= 1 ? 1 : (r_ij < t)                                      (uint64 arithmetic)
    syndromes  syndromes(i, r) = XOR over the stored entries (r, j) of H of errors(i, j) & 1
    score      d = (guesses ^ errors) & 1; flag bit 0: d != 0, bit 1: H d != 0, bit 2: L d != 0;
               counts = (columns, columns with bit 0, with bit 1, with bit 2)
"""
import numpy as np
import scipy.sparse as sp

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z: int) -> int:
    """The SplitMix64 finaliser on a Python int."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def mix_array(z: np.ndarray) -> np.ndarray:
    """The same on a uint64 array (numpy's uint64 arithmetic wraps)."""
    z = z.astype(np.uint64, copy=True)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def threshold(per: float) -> int:
    """t of the rule, for 0 <= per < 1: the product is a power-of-two scaling (exact), int() truncates."""
    assert 0.0 <= per < 1.0
    return int(per * 18446744073709551616.0)


def sample(n: int, batch: int, per: float, seed: int = 0, column0: int = 0) -> np.ndarray:
    """errors [batch][n] uint8."""
    if not (0.0 <= per <= 1.0):
        raise ValueError("per outside [0, 1]")
    if per >= 1.0:
        return np.ones((batch, n), dtype=np.uint8)
    keys = np.array([mix(seed + GOLDEN * (column0 + i + 1)) for i in range(batch)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = mix_array(keys[:, None] + np.arange(n, dtype=np.uint64)[None, :])
    return (r < np.uint64(threshold(per))).astype(np.uint8)


def _pattern(H) -> sp.csr_matrix:
    M = sp.csr_matrix(H)
    M = sp.csr_matrix((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape)   # every stored entry is an edge
    return M


def syndromes(H, errors_bn: np.ndarray) -> np.ndarray:
    """[batch][s] uint8."""
    M = _pattern(H)
    e = (np.asarray(errors_bn) & 1).astype(np.int64)
    return (np.asarray(M @ e.T) % 2).T.astype(np.uint8)


def score(H, L, guesses_bn: np.ndarray, errors_bn: np.ndarray):
    """-> (flags [batch] uint8, counts int64[4]).  L = None: no logical rows."""
    d = ((np.asarray(guesses_bn) ^ np.asarray(errors_bn)) & 1).astype(np.uint8)
    B = d.shape[0]
    flags = d.any(axis=1).astype(np.uint8)
    flags |= syndromes(H, d).any(axis=1).astype(np.uint8) << 1
    if L is not None and sp.csr_matrix(L).shape[0] > 0:
        flags |= syndromes(L, d).any(axis=1).astype(np.uint8) << 2
    counts = np.array([B, int((flags & 1).sum()), int(((flags >> 1) & 1).sum()), int(((flags >> 2) & 1).sum())], dtype=np.int64)
    return flags, counts
