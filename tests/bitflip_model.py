"""CPU model of the bit-flip decoder: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it.

A plain numpy restatement of `decode!(decoder::BitFlipDecoder, syndrome)` (src/decoders/iterative_bitflip.jl:116-157)
AS THE REFERENCE ORDERS IT: each iteration recomputes H * err mod 2, compares it with the syndrome, lets every check add
+1 (mismatched) or -1 (matched) to the votes of its bits, takes the maximum, and toggles one of the bits that hold it.
Deliberately not the incremental form the kernels use.  The votes are cleared once per syndrome (reset!, :84-88), not
per iteration.  The only freedom is the choice among the maximisers (`rand(max_idxs)`, :148): a pluggable `chooser`,
with the three rules of include/ldpc_mi355x.h as ready-made ones.
"""
import numpy as np
import scipy.sparse as sp

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
TIE_RANDOM, TIE_FIRST, TIE_LAST = 0, 1, 2


def mix(z: int) -> int:
    """The SplitMix64 finaliser, in uint64 arithmetic."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def random_rank(seed: int, column: int, it: int, k: int) -> int:
    """Candidate (0-based, in ascending bit order) of `k` that LDPC_BF_TIE_RANDOM takes for column number `column`
    (column0 + index in the call) in the 1-based iteration `it`."""
    r = mix(mix(seed + GOLDEN * (column + 1)) + it)
    return ((r >> 32) * k) >> 32


def chooser_for(tie_break: int, seed: int = 0):
    """chooser(column, it, candidates) -> bit index, for one of the header's rules."""
    if tie_break == TIE_FIRST:
        return lambda column, it, cand: int(cand[0])
    if tie_break == TIE_LAST:
        return lambda column, it, cand: int(cand[-1])
    assert tie_break == TIE_RANDOM
    return lambda column, it, cand: int(cand[random_rank(seed, column, it, len(cand))])


class BitFlipModel:
    def __init__(self, H, max_iters: int):
        M = sp.csr_matrix(H)
        M.eliminate_zeros()            # only entries whose stored value is true count (`sparse_H[i, j]`, `sparse_H * err`)
        M.sort_indices()
        self.H = sp.csr_matrix((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape)
        self.s, self.n = self.H.shape
        self.max_iters = int(max_iters)
        self.row_len = np.diff(self.H.indptr)

    def decode(self, syndrome, chooser, column: int = 0, trace=None):
        """-> (err [n] u8, converged bool, iterations entered, stop reason 0 | 1 | 2).  `trace`, a list, receives per
        flipping iteration (iteration, votes copy, candidates, chosen bit)."""
        H, s = self.H, self.s
        syndrome = np.asarray(syndrome).astype(np.int64).reshape(-1)
        assert syndrome.size == s
        err = np.zeros(self.n, dtype=np.int64)
        votes = np.zeros(self.n, dtype=np.int64)
        for it in range(1, self.max_iters + 1):
            syn = np.asarray(H @ err).reshape(-1) % 2
            if np.array_equal(syn, syndrome):               # an entry other than 0/1 can never be equal
                return err.astype(np.uint8), True, it, 1
            # the loop over the checks (:131-143), check after check in one unbuffered scatter-add: every edge (i, j)
            # adds +1 to votes[j] when check i is mismatched and -1 when it is matched
            np.add.at(votes, H.indices, np.repeat(np.where(syn != syndrome, 1, -1), self.row_len))
            if self.n == 0 or votes.max() < 0:              # (no bit at all: the library reports reason 2 as well)
                return err.astype(np.uint8), True, it, 2
            cand = np.nonzero(votes == votes.max())[0]
            j = chooser(column, it, cand)
            if trace is not None:
                trace.append((it, votes.copy(), cand.copy(), j))
            err[j] = 1 - err[j]
        return err.astype(np.uint8), False, self.max_iters, 0

    def decode_batch(self, syn_bs, tie_break: int = TIE_RANDOM, seed: int = 0, column0: int = 0):
        """syn [B][s] -> (errors [B][n] u8, converged [B] u8, iters [B] i32, stop_reason [B] u8), column i as column0 + i."""
        syn_bs = np.asarray(syn_bs)
        B = syn_bs.shape[0]
        ch = chooser_for(tie_break, seed)
        err = np.zeros((B, self.n), dtype=np.uint8)
        conv = np.zeros(B, dtype=np.uint8)
        its = np.zeros(B, dtype=np.int32)
        stop = np.zeros(B, dtype=np.uint8)
        for i in range(B):
            err[i], c, its[i], stop[i] = self.decode(syn_bs[i], ch, column0 + i)
            conv[i] = c
        return err, conv, its, stop
