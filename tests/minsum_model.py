"""CPU model of the normalised min-sum decoder: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it and
nothing here calls the library.  A numpy float32 restatement of THE RULE of include/ldpc_mi355x.h (the ldpc_minsum_*
section), written from the header: it loops over the edges and is vectorised over the batch, every operation is one
float32 operation (numpy rounds each once, nothing is fused), and a column that has stopped is frozen.

    b_k = min(max(L[j_k] - c[i][j_k], -clip), clip); neg_k = b_k < 0; mag_k = |b_k|
    m1 = m2 = clip, a = none; k ascending: mag_k < m1 -> m2 = m1, m1 = mag_k, a = k; else mag_k < m2 -> m2 = mag_k
    par = syndrome_i ^ XOR neg_k; c[i][j_k] = alpha * (k == a ? m2 : m1), sign bit set iff par ^ neg_k
    L[j] = channel_llr[j] + c[i_0][j] + c[i_1][j] + ... (ascending checks); err[j] = L[j] <= 0; stop if H err == syndrome
"""
import numpy as np
import scipy.sparse as sp

F = np.float32


def llr_of_probs(p) -> np.ndarray:
    """channel_llr as MinSumDecoder computes it from error probabilities: float64 log((1 - p) / p), rounded to float32."""
    p = np.asarray(p, dtype=np.float64)
    return np.log((1.0 - p) / p).astype(np.float32)


class MinSumModel:
    def __init__(self, H, channel_llr, max_iters: int, alpha: float = 0.75, clip: float = 1e6):
        M = sp.csr_matrix(H)
        M = sp.csr_matrix((np.ones(M.nnz, dtype=np.int8), M.indices, M.indptr), shape=M.shape)   # every stored entry is an edge
        M.sort_indices()
        self.s, self.n = M.shape
        self.rows = [M.indices[M.indptr[i]:M.indptr[i + 1]].astype(np.int64) for i in range(self.s)]   # bits of a check, ascending
        C = sp.csc_matrix(M)
        C.sort_indices()
        self.cols = [C.indices[C.indptr[j]:C.indptr[j + 1]].astype(np.int64) for j in range(self.n)]   # checks of a bit, ascending
        self.pos = {(i, int(j)): k for i in range(self.s) for k, j in enumerate(self.rows[i])}
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
            newL = np.tile(self.prior, (B, 1))
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
