"""CPU model of the guided-decimation min-sum decoder: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it
and nothing here calls the library.  A numpy float32 restatement of THE RULE of include/ldpc_mi355x.h (the ldpc_decim_*
section), written from the header on top of the graph arrays of MinSumModel: vectorised over the batch, every operation
is one float32 operation, and a column that has stopped is frozen -- never written again.

    iteration t: check sweep on L (the min-sum rule; a pinned bit enters like any other)
                 bit sweep: the pending bit takes its pin; every other bit outside D is the min-sum sum; D is left alone
                 test: H err == syndrome -> converged, stop
                 t % T == 0 and not matched: |D| == Dmax -> stop; else j* = argmax |L| outside D (lowest index on a tie),
                 negative = L[j*] <= 0, j* joins D and is pending: check sweep t + 1 still reads L[j*] as it is

Two additions serve the tests of the tie rule alone: `tie="highest"` restates the rule with the HIGHEST index on a tie (what a
kernel that breaks ties wrongly would compute; the default "lowest" is the rule), and `last_ties` counts, over the last
decode, the decimations in which at least two bits outside D shared the largest |L| -- the decimations where the two differ.
"""
import numpy as np

from minsum_model import MinSumModel

F = np.float32


class DecimModel(MinSumModel):
    def __init__(self, H, channel_llr, round_iters: int, max_decimations: int, alpha: float = 0.75, clip: float = 1e6,
                 tie: str = "lowest"):
        super().__init__(H, channel_llr, round_iters, alpha, clip)
        assert tie in ("lowest", "highest")
        self.tie, self.last_ties = tie, 0
        self.round_iters, self.max_dec = int(round_iters), int(max_decimations)
        assert self.round_iters >= 0 and 0 <= self.max_dec <= self.n
        self.pin = F(2.0) * self.clip
        assert np.isfinite(self.pin)

    def decode(self, syn_bs):
        """syn [B][s] -> (err [B][n] u8, conv [B] u8, iters [B] i32, decimated [B] i32, L [B][n] f32)."""
        y = (np.asarray(syn_bs).reshape(-1, self.s) != 0)
        B, n, T = y.shape[0], self.n, self.round_iters
        self.last_ties = 0
        if T == 0:
            return (np.zeros((B, n), np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, n), F))
        alpha, clip = self.alpha, self.clip
        L = np.tile(self.prior, (B, 1))
        c = [np.zeros((B, len(r)), dtype=F) for r in self.rows]
        D = np.zeros((B, n), dtype=bool)
        pending = np.full(B, -1, dtype=np.int64)      # j*, or -1
        negative = np.zeros(B, dtype=bool)
        active = np.ones(B, dtype=bool)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        rows_b = np.arange(B)
        t = 0
        while active.any():
            t += 1
            # 1. check sweep (the rule of minsum_model.py, on L)
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
            # 2. bit sweep: the pending pin, the sums outside D, nothing inside D
            newL = np.tile(self.prior, (B, 1))
            for j, rs in enumerate(self.cols):
                for i in rs:
                    newL[:, j] = newL[:, j] + c[i][:, self.pos[(int(i), j)]]
            write = active[:, None] & ~D
            L[write] = newL[write]
            has = active & (pending >= 0)
            L[rows_b[has], pending[has]] = np.where(negative[has], -self.pin, self.pin)
            pending[has] = -1
            iters[active] = t
            # 3. test
            err = L <= 0
            matched = np.ones(B, dtype=bool)
            for i, r in enumerate(self.rows):
                matched &= (err[:, r].sum(axis=1) % 2 == 1) == y[:, i]
            stop = active & matched
            conv[stop] = 1
            active &= ~stop
            # 4. end of a round
            if t % T == 0 and active.any():
                nd = D.sum(axis=1)
                active &= ~(nd == self.max_dec)
                if active.any():
                    mag = np.where(D, F(-1.0), np.abs(L))     # outside D only; argmax takes the lowest index on a tie
                    jstar = np.argmax(mag, axis=1)
                    if self.tie == "highest":
                        jstar = n - 1 - np.argmax(mag[:, ::-1], axis=1)
                    self.last_ties += int(((mag == mag.max(axis=1, keepdims=True)).sum(axis=1) >= 2)[active].sum())
                    rows_a = rows_b[active]
                    assert not D[rows_a, jstar[active]].any()
                    negative[active] = L[rows_a, jstar[active]] <= 0
                    pending[active] = jstar[active]
                    D[rows_a, jstar[active]] = True
        assert L.dtype == F and np.all(np.isfinite(L)) and not (pending >= 0).any()
        self.last_D = D      # [B][n] bool: the decimated bits of this decode, for the tests that look at the pins
        return (L <= 0).astype(np.uint8), conv, iters, D.sum(axis=1).astype(np.int32), L
