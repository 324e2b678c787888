"""CPU model of the CSS-code Monte-Carlo trial steps: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it
and nothing here calls the library.  A plain numpy restatement of the three rules of include/ldpc_mi355x.h:

    sample     k_i = mix(seed + GOLDEN * (column0 + i + 1)), r_ij = mix(k_i + j)                       (uint64 arithmetic)
               tx, ty, tz = (uint64)(px * 2^64), ...; a = tx, b = tx + ty, c = tx + ty + tz (an overflow is an error)
               Pauli(i, j) = X if r < a, Y if a <= r < b, Z if b <= r < c, else I;  ex = X or Y, ez = Y or Z
    syndromes  sz = Hz ex mod 2, sx = Hx ez mod 2 (stored entries are the edges, low bits count)
    score      dx = gx ^ ex, dz = gz ^ ez; bit 0: dx != 0 or dz != 0; bit 1: Hz dx != 0 or Hx dz != 0;
               bit 2: Lz dx != 0; bit 3: Lx dz != 0;
               counts = (columns, with bit 0, with bit 1, with bit 2 or 3, with bit 2, with bit 3)
"""
import numpy as np
import scipy.sparse as sp

import trials_model as tm

PAULI_I, PAULI_X, PAULI_Y, PAULI_Z = 0, 1, 2, 3


def rates_of(p):
    """A float is depolarizing noise (p / 3 each), a triple is itself."""
    if isinstance(p, (tuple, list)):
        return tuple(float(x) for x in p)
    return (float(p) / 3.0,) * 3


def thresholds(px: float, py: float, pz: float):
    """(a, b, c) of the rule as Python ints; ValueError for a bad rate or an overflow of either sum."""
    ts = []
    for r in (px, py, pz):
        if not (0.0 <= r < 1.0):       # (False for NaN as well)
            raise ValueError("rate outside [0, 1)")
        ts.append(int(r * 18446744073709551616.0))
    a, b, c = ts[0], ts[0] + ts[1], ts[0] + ts[1] + ts[2]
    if b > tm.MASK or c > tm.MASK:
        raise ValueError("a sum of the thresholds overflows 64 bits")
    return a, b, c


def paulis(n: int, batch: int, p, seed: int = 0, column0: int = 0) -> np.ndarray:
    """[batch][n] uint8 of PAULI_I / X / Y / Z: every qubit has exactly one."""
    a, b, c = thresholds(*rates_of(p))
    keys = np.array([tm.mix(seed + tm.GOLDEN * (column0 + i + 1)) for i in range(batch)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = tm.mix_array(keys[:, None] + np.arange(n, dtype=np.uint64)[None, :])
    a, b, c = np.uint64(a), np.uint64(b), np.uint64(c)
    out = np.full((batch, n), PAULI_I, dtype=np.uint8)
    out[r < c] = PAULI_Z
    out[r < b] = PAULI_Y
    out[r < a] = PAULI_X
    return out


def sample(n: int, batch: int, p, seed: int = 0, column0: int = 0):
    """-> (ex, ez), each [batch][n] uint8."""
    P = paulis(n, batch, p, seed, column0)
    return ((P == PAULI_X) | (P == PAULI_Y)).astype(np.uint8), ((P == PAULI_Y) | (P == PAULI_Z)).astype(np.uint8)


def syndromes(Hx, Hz, ex: np.ndarray, ez: np.ndarray):
    """-> (sx [batch][rows of Hx], sz [batch][rows of Hz])."""
    return tm.syndromes(Hx, ez), tm.syndromes(Hz, ex)


def _any_row(M, d: np.ndarray) -> np.ndarray:
    if M is None or sp.csr_matrix(M).shape[0] == 0:
        return np.zeros(d.shape[0], dtype=np.uint8)
    return tm.syndromes(M, d).any(axis=1).astype(np.uint8)


def score(Hx, Hz, Lx, Lz, gx, gz, ex, ez):
    """-> (flags [batch] uint8, counts int64[6]).  Lx / Lz = None: no such logical rows."""
    dx = ((np.asarray(gx) ^ np.asarray(ex)) & 1).astype(np.uint8)
    dz = ((np.asarray(gz) ^ np.asarray(ez)) & 1).astype(np.uint8)
    B = dx.shape[0]
    flags = (dx.any(axis=1) | dz.any(axis=1)).astype(np.uint8)
    flags |= (_any_row(Hz, dx) | _any_row(Hx, dz)) << 1
    flags |= _any_row(Lz, dx) << 2
    flags |= _any_row(Lx, dz) << 3
    bit = lambda k: (flags >> k) & 1   # noqa: E731
    counts = np.array([B, int(bit(0).sum()), int(bit(1).sum()), int((bit(2) | bit(3)).sum()), int(bit(2).sum()), int(bit(3).sum())],
                      dtype=np.int64)
    return flags, counts
