"""CPU model of the joint Pauli min-sum decoder of a general stabilizer code: test infrastructure, nothing under
ldpcdecoders.jl_amd/ imports it and nothing here calls the library.  A numpy float32 restatement of THE RULE of
include/ldpc_mi355x_stab.h, written from the header: it loops over the edges and is vectorised over the batch, every
operation is one float32 operation (numpy rounds each once, nothing is fused), and a column that has stopped is frozen.

    edge (i, j): type X (only Sx stores it), Z (only Sz), Y (both); s_i = XOR over the check's edges of ez_j (X-type),
                 ex_j (Z-type), ex_j ^ ez_j (Y-type)
    MX, MY, MZ [j]: the sums of the messages of the qubit's X-, Y-, Z-type edges, from +0;   min(x, y) = x < y ? x : y
    GX = (prior_x + MZ) + MY;  GY = (prior_y + MZ) + MX;  GZ = (prior_z + MX) + MY
    X-type: u = min(GY, GZ), w = GX < 0 ? GX : +0;  Z-type: u = min(GY, GX), w = GZ < 0 ? GZ : +0;
    Y-type: u = min(GX, GZ), w = GY < 0 ? GY : +0
    b_k = min(max((u_k - c[i][j_k]) - w_k, -clip), clip); neg_k, mag_k, m1, m2, a, par, new c: as the min-sum rule
    MX[j] = ((+0 + c[i_0][j]) + ...) over the X-type edges of j in ascending check order; MY, MZ the same
    best = X, g = GX; GZ < g -> Z; GY < g -> Y; E = g <= 0 ? best : I; ex = E in {X, Y}; ez = E in {Z, Y}
    stop if every check's XOR of anticommutations equals its entry (an empty check: only a 0 entry)
"""
import numpy as np
import scipy.sparse as sp

from pauli_model import PauliMinSumModel, _min, _pattern

F = np.float32
TX, TZ, TY = 1, 2, 3   # the type of an edge: bit 0 = the stabilizer has an X part there, bit 1 = a Z part


def symplectic_syndromes(Sx, Sz, ex, ez) -> np.ndarray:
    """ex, ez [B][n] -> [B][r] uint8: Sx ez ^ Sz ex over GF(2)."""
    A, B = sp.csr_matrix(_pattern(Sx), dtype=np.int64), sp.csr_matrix(_pattern(Sz), dtype=np.int64)
    ex, ez = np.asarray(ex, dtype=np.int64), np.asarray(ez, dtype=np.int64)
    return ((np.asarray(A @ ez.T) + np.asarray(B @ ex.T)) % 2).T.astype(np.uint8)


class StabMinSumModel:
    def __init__(self, Sx, Sz, priors, max_iters: int, alpha: float = 0.75, clip: float = 1e6):
        """priors: (prior_x, prior_y, prior_z), each [n] float32 and finite."""
        Mx, Mz = _pattern(Sx), _pattern(Sz)
        assert Mx.shape == Mz.shape
        self.r, self.n = Mx.shape
        T = sp.csr_matrix(Mx.astype(np.int8) + 2 * Mz.astype(np.int8))   # the union, its data the edge types
        T.sort_indices()
        self.rows = [T.indices[T.indptr[i]:T.indptr[i + 1]].astype(np.int64) for i in range(self.r)]   # qubits of a check, ascending
        self.types = [T.data[T.indptr[i]:T.indptr[i + 1]].astype(np.int64) for i in range(self.r)]
        assert all(set(t.tolist()) <= {TX, TZ, TY} for t in self.types)
        C = sp.csc_matrix(T)
        C.sort_indices()
        self.cols = [C.indices[C.indptr[j]:C.indptr[j + 1]].astype(np.int64) for j in range(self.n)]   # checks of a qubit, ascending
        self.col_types = [C.data[C.indptr[j]:C.indptr[j + 1]].astype(np.int64) for j in range(self.n)]
        self.pos = {(i, int(j)): k for i in range(self.r) for k, j in enumerate(self.rows[i])}
        self.px, self.py, self.pz = (np.asarray(t, dtype=F).reshape(self.n) for t in priors)
        assert all(np.all(np.isfinite(t)) for t in (self.px, self.py, self.pz))
        self.max_iters, self.alpha, self.clip = int(max_iters), F(alpha), F(clip)

    def _beliefs(self, MX, MY, MZ):
        return (self.px[None, :] + MZ) + MY, (self.py[None, :] + MZ) + MX, (self.pz[None, :] + MX) + MY

    _decide = staticmethod(PauliMinSumModel._decide)

    def _anticommutes(self, ex, ez, i):
        """[B] bool: the XOR over the edges of check i."""
        r, ty = self.rows[i], self.types[i]
        bits = (ez[:, r] & ((ty & 1) != 0)[None, :]) ^ (ex[:, r] & ((ty & 2) != 0)[None, :])
        return bits.sum(axis=1) % 2 == 1

    def decode(self, s_b):
        """s [B][r] -> (gx [B][n] u8, gz [B][n] u8, conv [B] u8, iters [B] i32, G [B][3][n] f32)."""
        y = np.asarray(s_b).reshape(-1, self.r) != 0
        B = y.shape[0]
        if self.max_iters == 0:
            return (np.zeros((B, self.n), np.uint8), np.zeros((B, self.n), np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int32),
                    np.zeros((B, 3, self.n), F))
        alpha, clip = self.alpha, self.clip
        M = [np.zeros((B, self.n), dtype=F) for _ in range(3)]   # MX, MY, MZ
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        active = np.ones(B, dtype=bool)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.full(B, self.max_iters, dtype=np.int32)
        zero = F(0.0)
        for t in range(1, self.max_iters + 1):
            GX, GY, GZ = self._beliefs(*M)
            for i, r in enumerate(self.rows):
                if len(r) == 0:
                    continue
                ty = self.types[i][None, :]
                gx, gy, gz = GX[:, r], GY[:, r], GZ[:, r]
                u = np.where(ty == TX, _min(gy, gz), np.where(ty == TZ, _min(gy, gx), _min(gx, gz)))
                own = np.where(ty == TX, gx, np.where(ty == TZ, gz, gy))
                w = np.where(own < 0, own, zero)
                b = np.minimum(np.maximum((u - c[i]) - w, -clip), clip)
                assert b.dtype == F
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
                at_a = np.arange(len(r))[None, :] == a[:, None]
                val = (alpha * np.where(at_a, m2[:, None], m1[:, None])).astype(F)
                c[i] = np.where(par[:, None] ^ neg, -val, val).astype(F)     # -(+0) is -0: the sign bit
            new = [np.zeros((B, self.n), dtype=F) for _ in range(3)]
            for j, rs in enumerate(self.cols):
                for i, ty in zip(rs, self.col_types[j]):
                    tot = new[{TX: 0, TY: 1, TZ: 2}[int(ty)]]
                    tot[:, j] = tot[:, j] + c[i][:, self.pos[(int(i), j)]]
            for k in range(3):
                M[k][active] = new[k][active]
            ex, ez = self._decide(*self._beliefs(*M))
            matched = np.ones(B, dtype=bool)
            for i in range(self.r):
                matched &= self._anticommutes(ex, ez, i) == y[:, i]
            stop = active & matched
            conv[stop] = 1
            iters[stop] = t
            active &= ~stop
            if not active.any():
                break
        self.last_messages = c                      # (a hook for the tests: the messages c[i] [B][degree] at the end)
        GX, GY, GZ = self._beliefs(*M)
        G = np.stack([GX, GY, GZ], axis=1)
        assert G.dtype == F and np.all(np.isfinite(G))
        ex, ez = self._decide(GX, GY, GZ)
        return ex.astype(np.uint8), ez.astype(np.uint8), conv, iters, G
