"""CPU model of the Pauli relay min-sum decoder: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it and
nothing here calls the library.  A numpy float32 restatement of THE RULE of include/ldpc_mi355x.h (the ldpc_pauli_relay_*
section), written from the header: the check sweep and the decision of tests/pauli_model.py, the leg bookkeeping of
tests/relay_model.py, vectorised over the batch with a leg index per column, every operation one float32 operation (numpy
rounds each once, nothing is fused), and a column that has stopped is frozen.

    g0W[r] = (1 - gamma[r]) * prior_W;  qW = rint(clamp(prior_W, +-2^24) * 2^16) as int64        (W = X, Y, Z)
    leg start: c = +0, TX = TZ = +0
    LambdaW = g0W[r] + gamma[r] * MW;  GX = LambdaX + TX;  GZ = LambdaZ + TZ;  GY = (LambdaY + TX) + TZ
    check sweep: the Pauli one on these G (Lambda from the M that stands)
    bit sweep: new TX, TZ from +0;  MX = LambdaX + TX, MZ = LambdaZ + TZ, MY = (LambdaY + TX) + TZ with Lambda from the OLD M
    decision on (MX, MY, MZ);  Hz ex == sz and Hx ez == sx: w = sum of qX / qY / qZ by the Pauli; lighter than best (or
    first) -> best; found += 1; found == stop_after -> stop, else the next leg starts from this M.  A leg of 0 iterations
    is skipped.
"""
import numpy as np

from pauli_model import PauliMinSumModel, _min
from relay_model import weights_of

F = np.float32


class PauliRelayModel(PauliMinSumModel):
    def __init__(self, Hx, Hz, priors, gammas, leg_iters, alpha: float = 0.75, clip: float = 1e6, stop_after: int = 1):
        """priors: (prior_x, prior_y, prior_z), each [n] float32 and finite; gammas [legs][n]; leg_iters [legs]."""
        super().__init__(Hx, Hz, priors, 0, alpha, clip)   # the graph in both orders, the priors, alpha and clip as float32
        self.leg_iters = np.asarray(leg_iters, dtype=np.int64).reshape(-1)
        self.legs = len(self.leg_iters)
        self.gammas = np.asarray(gammas, dtype=F).reshape(self.legs, self.n)
        assert self.legs >= 1 and (self.leg_iters >= 0).all() and stop_after >= 1
        assert np.all(np.isfinite(self.gammas)) and np.all(np.abs(self.gammas) < 1)
        one_minus = F(1.0) - self.gammas
        self.g0 = tuple((one_minus * p[None, :]).astype(F) for p in (self.px, self.py, self.pz))   # g0X, g0Y, g0Z [legs][n]
        self.q = tuple(weights_of(p) for p in (self.px, self.py, self.pz))                       # qX, qY, qZ
        self.stop_after = int(stop_after)

    def decode(self, sx_b, sz_b, trace=None):
        """sx [B][rx], sz [B][rz] -> (gx [B][n] u8, gz [B][n] u8, conv [B] u8, iters [B] i32, solutions [B] i32,
        M [B][3][n] f32: the planes MX, MY, MZ).
        trace: a list that receives (leg [B], iterations done in it [B], hit [B]) after every iteration."""
        yx = np.asarray(sx_b).reshape(-1, self.rx) != 0
        yz = np.asarray(sz_b).reshape(-1, self.rz) != 0
        assert yx.shape[0] == yz.shape[0]
        y = np.concatenate([yx, yz], axis=1)
        B, n = y.shape[0], self.n
        run = [r for r in range(self.legs) if self.leg_iters[r] > 0]   # a leg of 0 iterations is skipped
        iters = np.zeros(B, dtype=np.int32)
        found = np.zeros(B, dtype=np.int32)
        if not run:
            return (np.zeros((B, n), np.uint8), np.zeros((B, n), np.uint8), np.zeros(B, np.uint8), iters, found,
                    np.zeros((B, 3, n), F))
        alpha, clip, zero = self.alpha, self.clip, F(0.0)
        MX, MY, MZ = (np.tile(p, (B, 1)) for p in (self.px, self.py, self.pz))
        TX, TZ = np.zeros((B, n), dtype=F), np.zeros((B, n), dtype=F)
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        at = np.zeros(B, dtype=np.int64)       # position of the column's leg in `run`
        t = np.zeros(B, dtype=np.int64)        # iterations done in that leg
        start = np.ones(B, dtype=bool)
        active = np.ones(B, dtype=bool)
        best_x, best_z = np.zeros((B, n), dtype=bool), np.zeros((B, n), dtype=bool)
        best_w = np.zeros(B, dtype=np.int64)
        while active.any():
            leg = np.asarray(run)[at]
            Gm = self.gammas[leg]
            G0X, G0Y, G0Z = (g[leg] for g in self.g0)
            st = active & start
            if st.any():   # leg start
                for ci in c:
                    ci[st] = zero
                TX[st], TZ[st] = zero, zero
                t[st] = 0
                start[st] = False
            # Lambda from the M that stands, and the G of the check sweep
            LX, LY, LZ = G0X + Gm * MX, G0Y + Gm * MY, G0Z + Gm * MZ
            GX, GZ, GY = LX + TX, LZ + TZ, (LY + TX) + TZ
            assert GX.dtype == F and GY.dtype == F and GZ.dtype == F
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
                new = np.where(par[:, None] ^ neg, -val, val).astype(F)     # -(+0) is -0: the sign bit
                c[i] = np.where(active[:, None], new, c[i])
            newX, newZ = np.zeros((B, n), dtype=F), np.zeros((B, n), dtype=F)
            for j, rs in enumerate(self.cols):
                for i in rs:
                    m = c[i][:, self.pos[(int(i), j)]]
                    if i < self.rx:
                        newZ[:, j] = newZ[:, j] + m
                    else:
                        newX[:, j] = newX[:, j] + m
            nMX, nMZ, nMY = LX + newX, LZ + newZ, (LY + newX) + newZ      # Lambda from the old M
            assert nMX.dtype == F and nMY.dtype == F and nMZ.dtype == F
            TX[active], TZ[active] = newX[active], newZ[active]
            MX[active], MY[active], MZ[active] = nMX[active], nMY[active], nMZ[active]
            t[active] += 1
            iters[active] += 1
            ex, ez = self._decide(MX, MY, MZ)
            matched = np.ones(B, dtype=bool)
            for i, r in enumerate(self.rows):
                part = ez if i < self.rx else ex
                matched &= (part[:, r].sum(axis=1) % 2 == 1) == y[:, i]
            hit = active & matched
            qX, qY, qZ = self.q
            w = ((ex & ~ez) * qX[None, :] + (ex & ez) * qY[None, :] + (~ex & ez) * qZ[None, :]).sum(axis=1)
            better = hit & ((found == 0) | (w < best_w))   # a tie keeps the earlier solution
            best_x[better], best_z[better] = ex[better], ez[better]
            best_w[better] = w[better]
            found[hit] += 1
            if trace is not None:
                trace.append((leg.copy(), t.copy(), hit.copy()))
            stop = hit & (found == self.stop_after)
            leg_end = active & ~stop & (hit | (t == self.leg_iters[leg]))
            at[leg_end] += 1
            start[leg_end] = True
            stop |= leg_end & (at >= len(run))
            at[at >= len(run)] = len(run) - 1
            active &= ~stop
        M = np.stack([MX, MY, MZ], axis=1)
        assert M.dtype == F and np.all(np.isfinite(M))
        have = found > 0
        ex, ez = self._decide(MX, MY, MZ)
        gx = np.where(have[:, None], best_x, ex).astype(np.uint8)
        gz = np.where(have[:, None], best_z, ez).astype(np.uint8)
        return gx, gz, have.astype(np.uint8), iters, found, M
