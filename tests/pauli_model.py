"""CPU model of the joint X/Z (Pauli) min-sum decoder: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it
and nothing here calls the library.  A numpy float32 restatement of THE RULE of include/ldpc_mi355x.h (the
ldpc_pauli_minsum_* section), written from the header: it loops over the edges and is vectorised over the batch, every
operation is one float32 operation (numpy rounds each once, nothing is fused), and a column that has stopped is frozen.

    checks: Hx rows 0 .. rx - 1 (they see Z parts), then Hz rows rx .. rx + rz - 1 (they see X parts)
    GX = prior_x + TX; GZ = prior_z + TZ; GY = (prior_y + TX) + TZ;   min(x, y) = x < y ? x : y
    Hx row: u = min(GY, GZ), w = GX < 0 ? GX : +0;   Hz row: u = min(GY, GX), w = GZ < 0 ? GZ : +0
    b_k = min(max((u_k - c[i][j_k]) - w_k, -clip), clip); neg_k, mag_k, m1, m2, a, par, new c: as the min-sum rule
    TX[j] = ((+0 + c[i_0][j]) + ...) over the Hz checks of j, TZ[j] over its Hx checks (ascending)
    best = X, g = GX; GZ < g -> Z; GY < g -> Y; E = g <= 0 ? best : I; ex = E in {X, Y}; ez = E in {Z, Y}
    stop if Hz ex == sz and Hx ez == sx
"""
import numpy as np
import scipy.sparse as sp

F = np.float32


def pauli_priors(probs) -> np.ndarray:
    """[n][3] (px, py, pz) -> [3][n] float32 as PauliMinSumDecoder computes them: float64 log((1 - px - py - pz) / pW)."""
    q = np.asarray(probs, dtype=np.float64).reshape(-1, 3)
    rest = 1.0 - q[:, 0] - q[:, 1] - q[:, 2]
    return np.log(rest[None, :] / q.T).astype(np.float32)


def depolarizing_priors(n: int, p) -> np.ndarray:
    """The three tables of a uniform `p` (a float: p / 3 each; a triple is itself)."""
    rates = tuple(float(x) for x in p) if isinstance(p, (tuple, list)) else (float(p) / 3.0,) * 3
    return pauli_priors(np.tile(np.array(rates, dtype=np.float64), (n, 1)))


def _pattern(H):
    M = sp.csr_matrix(H)
    M = sp.csr_matrix((np.ones(M.nnz, dtype=np.int8), M.indices, M.indptr), shape=M.shape)   # every stored entry is an edge
    M.sort_indices()
    return M


def _min(x, y):
    return np.where(x < y, x, y)


class PauliMinSumModel:
    def __init__(self, Hx, Hz, priors, max_iters: int, alpha: float = 0.75, clip: float = 1e6):
        """priors: (prior_x, prior_y, prior_z), each [n] float32 and finite."""
        Mx, Mz = _pattern(Hx), _pattern(Hz)
        assert Mx.shape[1] == Mz.shape[1]
        self.rx, self.rz, self.n = Mx.shape[0], Mz.shape[0], Mx.shape[1]
        self.s = self.rx + self.rz
        M = sp.csr_matrix(sp.vstack([Mx, Mz]))
        M.sort_indices()
        self.rows = [M.indices[M.indptr[i]:M.indptr[i + 1]].astype(np.int64) for i in range(self.s)]   # qubits of a check, ascending
        C = sp.csc_matrix(M)
        C.sort_indices()
        self.cols = [C.indices[C.indptr[j]:C.indptr[j + 1]].astype(np.int64) for j in range(self.n)]   # checks of a qubit, ascending
        self.pos = {(i, int(j)): k for i in range(self.s) for k, j in enumerate(self.rows[i])}
        self.px, self.py, self.pz = (np.asarray(t, dtype=F).reshape(self.n) for t in priors)
        assert all(np.all(np.isfinite(t)) for t in (self.px, self.py, self.pz))
        self.max_iters, self.alpha, self.clip = int(max_iters), F(alpha), F(clip)

    def _beliefs(self, TX, TZ):
        return self.px[None, :] + TX, (self.py[None, :] + TX) + TZ, self.pz[None, :] + TZ

    @staticmethod
    def _decide(GX, GY, GZ):
        """-> (ex, ez) as bool arrays."""
        best = np.ones(GX.shape, dtype=np.int8)     # 1 = X, 2 = Z, 3 = Y: bit 0 the X part, bit 1 the Z part
        g = GX.copy()
        lt = GZ < g
        best[lt], g[lt] = 2, GZ[lt]
        lt = GY < g
        best[lt], g[lt] = 3, GY[lt]
        E = np.where(g <= 0, best, 0)
        return (E & 1) != 0, (E & 2) != 0

    def decode(self, sx_b, sz_b):
        """sx [B][rx], sz [B][rz] -> (gx [B][n] u8, gz [B][n] u8, conv [B] u8, iters [B] i32, G [B][3][n] f32)."""
        yx = np.asarray(sx_b).reshape(-1, self.rx) != 0
        yz = np.asarray(sz_b).reshape(-1, self.rz) != 0
        assert yx.shape[0] == yz.shape[0]
        y = np.concatenate([yx, yz], axis=1)
        B = y.shape[0]
        if self.max_iters == 0:
            return (np.zeros((B, self.n), np.uint8), np.zeros((B, self.n), np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int32),
                    np.zeros((B, 3, self.n), F))
        alpha, clip = self.alpha, self.clip
        TX, TZ = np.zeros((B, self.n), dtype=F), np.zeros((B, self.n), dtype=F)
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        active = np.ones(B, dtype=bool)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.full(B, self.max_iters, dtype=np.int32)
        zero = F(0.0)
        for t in range(1, self.max_iters + 1):
            GX, GY, GZ = self._beliefs(TX, TZ)
            for i, r in enumerate(self.rows):
                if len(r) == 0:
                    continue
                if i < self.rx:   # an Hx row sees the Z parts
                    u = _min(GY[:, r], GZ[:, r])
                    w = np.where(GX[:, r] < 0, GX[:, r], zero)
                else:             # an Hz row sees the X parts
                    u = _min(GY[:, r], GX[:, r])
                    w = np.where(GZ[:, r] < 0, GZ[:, r], zero)
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
                own = np.arange(len(r))[None, :] == a[:, None]
                val = (alpha * np.where(own, m2[:, None], m1[:, None])).astype(F)
                c[i] = np.where(par[:, None] ^ neg, -val, val).astype(F)     # -(+0) is -0: the sign bit
            newX, newZ = np.zeros((B, self.n), dtype=F), np.zeros((B, self.n), dtype=F)
            for j, rs in enumerate(self.cols):
                for i in rs:
                    m = c[i][:, self.pos[(int(i), j)]]
                    if i < self.rx:
                        newZ[:, j] = newZ[:, j] + m
                    else:
                        newX[:, j] = newX[:, j] + m
            TX[active], TZ[active] = newX[active], newZ[active]
            ex, ez = self._decide(*self._beliefs(TX, TZ))
            matched = np.ones(B, dtype=bool)
            for i, r in enumerate(self.rows):
                part = ez if i < self.rx else ex
                matched &= (part[:, r].sum(axis=1) % 2 == 1) == y[:, i]
            stop = active & matched
            conv[stop] = 1
            iters[stop] = t
            active &= ~stop
            if not active.any():
                break
        GX, GY, GZ = self._beliefs(TX, TZ)
        G = np.stack([GX, GY, GZ], axis=1)
        assert G.dtype == F and np.all(np.isfinite(G))
        ex, ez = self._decide(GX, GY, GZ)
        return ex.astype(np.uint8), ez.astype(np.uint8), conv, iters, G
