"""CPU model of the relay min-sum decoder: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it and nothing
here calls the library.  A numpy float32 restatement of THE RULE of include/ldpc_mi355x.h (the ldpc_relay_* section),
written from the header: vectorised over the batch with a leg index per column, every operation one float32 operation
(numpy rounds each once, nothing is fused), and a column that has stopped is frozen.

    g0[r] = (1 - gamma[r]) * llr;  q = rint(clamp(llr, +-2^24) * 2^16) as int64
    leg start: c = +0, X = g0[r] + gamma[r] * M
    check sweep: the min-sum one on X;  bit sweep: M = (g0[r] + gamma[r] * M) + c..., X = (g0[r] + gamma[r] * new M) + c...
    H (M <= 0) == syndrome: w = sum q[err]; lighter than best (or first) -> best; found += 1; found == stop_after -> stop,
    else the next leg starts from this M.  A leg of 0 iterations is skipped.
"""
import numpy as np

from minsum_model import MinSumModel

F = np.float32


def weights_of(channel_llr) -> np.ndarray:
    """q of the rule: the prior in units of 2^-16, clamped to +-2^24, as int64."""
    p = np.asarray(channel_llr, dtype=F).astype(np.float64)
    return np.rint(np.clip(p, -2.0 ** 24, 2.0 ** 24) * 65536.0).astype(np.int64)


class RelayModel:
    def __init__(self, H, channel_llr, gammas, leg_iters, alpha: float = 0.75, clip: float = 1e6, stop_after: int = 1):
        g = MinSumModel(H, channel_llr, 0, alpha, clip)   # the graph in both orders, the prior, alpha and clip as float32
        self.s, self.n, self.rows, self.cols, self.pos = g.s, g.n, g.rows, g.cols, g.pos
        self.prior, self.alpha, self.clip = g.prior, g.alpha, g.clip
        self.leg_iters = np.asarray(leg_iters, dtype=np.int64).reshape(-1)
        self.legs = len(self.leg_iters)
        self.gammas = np.asarray(gammas, dtype=F).reshape(self.legs, self.n)
        assert self.legs >= 1 and (self.leg_iters >= 0).all() and stop_after >= 1
        assert np.all(np.isfinite(self.gammas)) and np.all(np.abs(self.gammas) < 1)
        self.g0 = ((F(1.0) - self.gammas) * self.prior[None, :]).astype(F)
        self.q = weights_of(self.prior)
        self.stop_after = int(stop_after)

    def _sum_messages(self, start, c):
        """start[:, j] + c[i_0][j] + c[i_1][j] + ..., from the left, checks ascending."""
        out = start.copy()
        for j, rs in enumerate(self.cols):
            for i in rs:
                out[:, j] = out[:, j] + c[i][:, self.pos[(int(i), j)]]
        return out

    def decode(self, syn_bs, trace=None, steps=None):
        """syn [B][s] -> (err [B][n] u8, conv [B] u8, iters [B] i32, solutions [B] i32, M [B][n] f32).
        trace: a list that receives (iteration, leg [B], M, X, weight [B], hit [B]) after every iteration;
        steps: one that receives (leg [B], iterations done in it [B], hit [B]), the form of PauliRelayModel's trace."""
        y = (np.asarray(syn_bs).reshape(-1, self.s) != 0)
        B, n = y.shape[0], self.n
        run = [r for r in range(self.legs) if self.leg_iters[r] > 0]   # a leg of 0 iterations is skipped
        iters = np.zeros(B, dtype=np.int32)
        found = np.zeros(B, dtype=np.int32)
        if not run:
            return np.zeros((B, n), np.uint8), np.zeros(B, np.uint8), iters, found, np.zeros((B, n), F)
        alpha, clip = self.alpha, self.clip
        M = np.tile(self.prior, (B, 1))
        X = np.zeros((B, n), dtype=F)
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        at = np.zeros(B, dtype=np.int64)       # position of the column's leg in `run`
        t = np.zeros(B, dtype=np.int64)        # iterations done in that leg
        start = np.ones(B, dtype=bool)
        active = np.ones(B, dtype=bool)
        best = np.zeros((B, n), dtype=bool)
        best_w = np.zeros(B, dtype=np.int64)
        step = 0
        while active.any():
            step += 1
            leg = np.asarray(run)[at]
            G, G0 = self.gammas[leg], self.g0[leg]
            st = active & start
            if st.any():   # leg start
                X[st] = (G0 + G * M)[st]
                for ci in c:
                    ci[st] = F(0.0)
                t[st] = 0
                start[st] = False
            for i, r in enumerate(self.rows):
                if len(r) == 0:
                    continue
                b = np.minimum(np.maximum(X[:, r] - c[i], -clip), clip)
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
                new = np.where(par[:, None] ^ neg, -val, val).astype(F)     # -(+0) is -0: the sign bit
                c[i] = np.where(active[:, None], new, c[i])
            newM = self._sum_messages(G0 + G * M, c)          # Lambda from the old M
            newX = self._sum_messages(G0 + G * newM, c)       # Lambda' from the new M
            assert newM.dtype == F and newX.dtype == F
            M[active] = newM[active]
            X[active] = newX[active]
            t[active] += 1
            iters[active] += 1
            err = M <= 0
            matched = np.ones(B, dtype=bool)
            for i, r in enumerate(self.rows):
                matched &= (err[:, r].sum(axis=1) % 2 == 1) == y[:, i]
            hit = active & matched
            w = (err * self.q[None, :]).sum(axis=1)
            better = hit & ((found == 0) | (w < best_w))   # a tie keeps the earlier solution
            best[better] = err[better]
            best_w[better] = w[better]
            found[hit] += 1
            if trace is not None:
                trace.append((step, leg.copy(), M.copy(), X.copy(), w.copy(), hit.copy()))
            if steps is not None:
                steps.append((leg.copy(), t.copy(), hit.copy()))
            stop = hit & (found == self.stop_after)
            leg_end = active & ~stop & (hit | (t == self.leg_iters[leg]))
            at[leg_end] += 1
            start[leg_end] = True
            stop |= leg_end & (at >= len(run))
            at[at >= len(run)] = len(run) - 1
            active &= ~stop
        assert M.dtype == F and np.all(np.isfinite(M))
        have = found > 0
        err = np.where(have[:, None], best, M <= 0).astype(np.uint8)
        return err, have.astype(np.uint8), iters, found, M
