"""CPU model of the LAYERED schedule of the normalised min-sum decoder: test infrastructure, nothing under
ldpcdecoders.jl_amd/ imports it and nothing here calls the library.  A numpy float32 restatement of THE LAYERED RULE of
include/ldpc_mi355x.h (the ldpc_minsum_* section), written from the header, layer assignment included: it loops over the
layers and their checks and is vectorised over the batch, every operation is one float32 operation (numpy rounds each
once, nothing is fused), and a column that has stopped is frozen.

    layers: checks ascending; a check with no bits: none; else the lowest layer that holds no check sharing a bit with it
    per layer 0 .. K - 1, per check i of it (bits j_0 < j_1 < ...):
      b_k = min(max(L[j_k] - c[i][j_k], -clip), clip); neg_k = b_k < 0; mag_k = |b_k|
      m1 = m2 = clip, a = none; k ascending: mag_k < m1 -> m2 = m1, m1 = mag_k, a = k; else mag_k < m2 -> m2 = mag_k
      par = syndrome_i ^ XOR neg_k; c[i][j_k] = alpha * (k == a ? m2 : m1), sign bit set iff par ^ neg_k
      L[j_k] = b_k + c[i][j_k]
    after the last layer: err[j] = L[j] <= 0; stop if H err == syndrome
"""
import numpy as np
import scipy.sparse as sp

F = np.float32


def layers_of(H):
    """(layer_of [s] int32, -1 for a check with no bits; K) by first fit over the checks in ascending index."""
    M = sp.csr_matrix(H)
    M = sp.csr_matrix((np.ones(M.nnz, dtype=np.int8), M.indices, M.indptr), shape=M.shape)   # every stored entry is an edge
    s, n = M.shape
    bits_of_layer = []                                  # per layer: which bits its checks hold
    layer_of = np.full(s, -1, dtype=np.int32)
    for i in range(s):
        r = M.indices[M.indptr[i]:M.indptr[i + 1]]
        if r.size == 0:
            continue
        for k, taken in enumerate(bits_of_layer):
            if not taken[r].any():
                break
        else:
            k = len(bits_of_layer)
            bits_of_layer.append(np.zeros(n, dtype=bool))
        bits_of_layer[k][r] = True
        layer_of[i] = k
    return layer_of, len(bits_of_layer)


class LayeredMinSumModel:
    def __init__(self, H, channel_llr, max_iters: int, alpha: float = 0.75, clip: float = 1e6, layers=None):
        """layers: a list of lists of checks to use instead of the rule's (the model's own tests: one check per layer,
        a permutation inside a layer); None = first fit."""
        M = sp.csr_matrix(H)
        M = sp.csr_matrix((np.ones(M.nnz, dtype=np.int8), M.indices, M.indptr), shape=M.shape)
        M.sort_indices()
        self.s, self.n = M.shape
        self.rows = [M.indices[M.indptr[i]:M.indptr[i + 1]].astype(np.int64) for i in range(self.s)]   # bits of a check, ascending
        if layers is None:
            self.layer_of, self.K = layers_of(M)
            layers = [[i for i in range(self.s) if self.layer_of[i] == k] for k in range(self.K)]      # ascending inside a layer
        self.layers = [list(map(int, ly)) for ly in layers]
        self.K = len(self.layers)
        listed = sorted(i for ly in self.layers for i in ly)
        assert listed == [i for i in range(self.s) if len(self.rows[i])], "every non-empty check in exactly one layer"
        self.prior = np.asarray(channel_llr, dtype=F).reshape(self.n)
        assert np.all(np.isfinite(self.prior))
        self.max_iters, self.alpha, self.clip = int(max_iters), F(alpha), F(clip)

    def decode(self, syn_bs):
        """syn [B][s] -> (err [B][n] u8, conv [B] u8, iters [B] i32, L [B][n] f32)."""
        y = (np.asarray(syn_bs).reshape(-1, self.s) != 0)
        B = y.shape[0]
        if self.max_iters == 0:
            return (np.zeros((B, self.n), np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros((B, self.n), F))
        alpha, clip = self.alpha, self.clip
        L = np.tile(self.prior, (B, 1))
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
