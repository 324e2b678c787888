"""CPU model of min-sum decoding with PER-SYNDROME PRIORS: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports
it and nothing here calls the library.  Written from include/ldpc_mi355x.h (the ldpc_minsum_* section): column i is decoded
by THE RULE (flooding) or THE LAYERED RULE with every channel_llr[j] -- the initial L and the left-most addend of the
bit sweep -- replaced by priors[i][j].  The two models below are tests/minsum_model.py and tests/layered_model.py with
`np.tile(self.prior, (B, 1))` replaced by the matrix; every operation is one float32 operation.

    given bits    priors[i][j] = llr_if1[j] if given[i][j] & 1 else llr_if0[j]
    non-finite    a column that holds a NaN or an infinite prior is not decoded: err zeros, converged 0, iters 0, L 0
    conditional   the Z part of a qubit given its X part, rates (px, py, pz):
                  p_if1 = py / (px + py), p_if0 = pz / (1 - px - py), float64
"""
import numpy as np
import scipy.sparse as sp

from layered_model import LayeredMinSumModel
from minsum_model import MinSumModel

F = np.float32


def select_priors(given, llr_if0, llr_if1) -> np.ndarray:
    """[B][n] float32 from given [B][n] (the low bit counts) and the two tables [n]."""
    g = (np.asarray(given).astype(np.int64) & 1).astype(bool)
    return np.where(g, np.asarray(llr_if1, dtype=F)[None, :], np.asarray(llr_if0, dtype=F)[None, :]).astype(F)


def conditional_probs(p):
    """(p_if0, p_if1) of the Z part given the X part; p a float (depolarizing, p / 3 each) or a triple (px, py, pz)."""
    px, py, pz = (np.float64(x) for x in (p if isinstance(p, (tuple, list)) else (float(p) / 3.0,) * 3))
    if px + py == 0:
        raise ValueError("px + py = 0: no X part ever occurs")
    p_if1, p_if0 = py / (px + py), pz / (np.float64(1.0) - px - py)
    if not (0.0 < p_if0 < 1.0 and 0.0 < p_if1 < 1.0):
        raise ValueError("a conditional probability is not strictly inside (0, 1)")
    return float(p_if0), float(p_if1)


def _with_nonfinite_rule(decode_finite, syn_bs, priors, s, n):
    y = np.asarray(syn_bs).reshape(-1, s)
    pri = np.asarray(priors, dtype=F)
    B = y.shape[0]
    assert pri.shape == (B, n), (pri.shape, (B, n))
    err, conv = np.zeros((B, n), np.uint8), np.zeros(B, np.uint8)
    iters, L = np.zeros(B, np.int32), np.zeros((B, n), F)
    ok = np.isfinite(pri).all(axis=1)
    if ok.any():
        err[ok], conv[ok], iters[ok], L[ok] = decode_finite(y[ok], pri[ok])
    return err, conv, iters, L


class PriorsMinSumModel(MinSumModel):
    """THE RULE with a prior per syndrome and bit; `decode(syn [B][s], priors [B][n])`."""

    def __init__(self, H, max_iters: int, alpha: float = 0.75, clip: float = 1e6):
        super().__init__(H, np.zeros(sp.csr_matrix(H).shape[1], dtype=F), max_iters, alpha, clip)

    def decode(self, syn_bs, priors):
        return _with_nonfinite_rule(self._decode_finite, syn_bs, priors, self.s, self.n)

    def _decode_finite(self, y, pri):
        y = y != 0
        B = y.shape[0]
        if self.max_iters == 0:
            return (np.zeros((B, self.n), np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros((B, self.n), F))
        alpha, clip = self.alpha, self.clip
        L = pri.copy()
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        active = np.ones(B, dtype=bool)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.full(B, self.max_iters, dtype=np.int32)
        for t in range(1, self.max_iters + 1):
            for i, r in enumerate(self.rows):
                if len(r) == 0:
                    continue
                b = np.minimum(np.maximum(L[:, r] - c[i], -clip), clip)
                neg, mag = b < 0, np.abs(b)
                m1 = np.full(B, clip, dtype=F)
                m2 = np.full(B, clip, dtype=F)
                a = np.full(B, -1, dtype=np.int64)
                for k in range(len(r)):
                    lt1 = mag[:, k] < m1
                    lt2 = ~lt1 & (mag[:, k] < m2)
                    m2 = np.where(lt1, m1, np.where(lt2, mag[:, k], m2))
                    m1 = np.where(lt1, mag[:, k], m1)
                    a = np.where(lt1, k, a)
                par = y[:, i] ^ (neg.sum(axis=1) % 2 == 1)
                own = np.arange(len(r))[None, :] == a[:, None]
                val = (alpha * np.where(own, m2[:, None], m1[:, None])).astype(F)
                c[i] = np.where(par[:, None] ^ neg, -val, val).astype(F)     # -(+0) is -0: the sign bit
            newL = pri.copy()                                                # the left-most addend: the column's own prior
            for j, rs in enumerate(self.cols):
                for i in rs:
                    newL[:, j] = newL[:, j] + c[i][:, self.pos[(int(i), j)]]
            L[active] = newL[active]
            err = L <= 0
            matched = np.ones(B, dtype=bool)
            for i, r in enumerate(self.rows):
                matched &= (err[:, r].sum(axis=1) % 2 == 1) == y[:, i]
            stop = active & matched
            conv[stop] = 1
            iters[stop] = t
            active &= ~stop
            if not active.any():
                break
        assert L.dtype == F and np.all(np.isfinite(L))
        return (L <= 0).astype(np.uint8), conv, iters, L


class PriorsLayeredModel(LayeredMinSumModel):
    """THE LAYERED RULE with a prior per syndrome and bit; `decode(syn [B][s], priors [B][n])`."""

    def __init__(self, H, max_iters: int, alpha: float = 0.75, clip: float = 1e6, layers=None):
        super().__init__(H, np.zeros(sp.csr_matrix(H).shape[1], dtype=F), max_iters, alpha, clip, layers)

    def decode(self, syn_bs, priors):
        return _with_nonfinite_rule(self._decode_finite, syn_bs, priors, self.s, self.n)

    def _decode_finite(self, y, pri):
        y = y != 0
        B = y.shape[0]
        if self.max_iters == 0:
            return (np.zeros((B, self.n), np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros((B, self.n), F))
        alpha, clip = self.alpha, self.clip
        L = pri.copy()
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        active = np.ones(B, dtype=bool)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.full(B, self.max_iters, dtype=np.int32)
        for t in range(1, self.max_iters + 1):
            for layer in self.layers:
                for i in layer:
                    r = self.rows[i]
                    b = np.minimum(np.maximum(L[:, r] - c[i], -clip), clip)
                    neg, mag = b < 0, np.abs(b)
                    m1 = np.full(B, clip, dtype=F)
                    m2 = np.full(B, clip, dtype=F)
                    a = np.full(B, -1, dtype=np.int64)
                    for k in range(len(r)):
                        lt1 = mag[:, k] < m1
                        lt2 = ~lt1 & (mag[:, k] < m2)
                        m2 = np.where(lt1, m1, np.where(lt2, mag[:, k], m2))
                        m1 = np.where(lt1, mag[:, k], m1)
                        a = np.where(lt1, k, a)
                    par = y[:, i] ^ (neg.sum(axis=1) % 2 == 1)
                    own = np.arange(len(r))[None, :] == a[:, None]
                    val = (alpha * np.where(own, m2[:, None], m1[:, None])).astype(F)
                    new_c = np.where(par[:, None] ^ neg, -val, val).astype(F)     # -(+0) is -0: the sign bit
                    new_L = (b + new_c).astype(F)
                    c[i][active] = new_c[active]                                   # a stopped column is frozen
                    L[np.ix_(active, r)] = new_L[active]
            err = L <= 0
            matched = np.ones(B, dtype=bool)
            for i, r in enumerate(self.rows):
                matched &= (err[:, r].sum(axis=1) % 2 == 1) == y[:, i]
            stop = active & matched
            conv[stop] = 1
            iters[stop] = t
            active &= ~stop
            if not active.any():
                break
        assert L.dtype == F and np.all(np.isfinite(L))
        return (L <= 0).astype(np.uint8), conv, iters, L


def model_of(schedule, H, max_iters, alpha=0.75, clip=1e6):
    return (PriorsLayeredModel if schedule == "layered" else PriorsMinSumModel)(H, max_iters, alpha, clip)
