"""The graphs, syndromes and oracle results that tests/test_gpu_bpots_paths.py decodes on the GPU, built without one, so
that tests/test_bpots_oracle.py can hold the C oracle against its second witness (oracle/bpots_reference_py.py) on the
same inputs.  Everything here is computed once per process and never written to afterwards.

A large batch is built from a POOL of at most 48 distinct syndromes: the oracle decodes the pool, and a batch is a list of
pool indices (columns are decoded independently, so the expectation of a column is the oracle's result for its syndrome).
The oracle costs about 0.28 us per edge, iteration and syndrome."""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import BPOTSOracle


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


def csc(H):
    M = sp.csc_matrix(H).astype(np.uint8)
    M.eliminate_zeros()
    M.sort_indices()
    return M


def oracle_decode(H, per, iters, T, C, syn):
    M = csc(H)
    out = BPOTSOracle((M.indptr, M.indices), M.shape, per, iters, T, C).batchdecode(syn)
    for x in out:
        x.setflags(write=False)
    return out


class Pool:
    """Distinct syndromes of one graph with one parameter set, and the oracle's answer for each."""

    def __init__(self, H, per, iters, T, C, syn):
        self.H, self.per, self.iters, self.T, self.C = csc(H), float(per), int(iters), int(T), float(C)
        self.syn = np.ascontiguousarray(syn, dtype=np.uint8)
        self.syn.setflags(write=False)
        self.err, self.conv, self.its = oracle_decode(self.H, per, iters, T, C, self.syn)
        # the order batches draw from (each where the pool has one): a syndrome with an entry above 1 first -- it can never
        # be matched, so it runs to max_iters --, a converged one second, a second wild one, one that ran past T unconverged
        # with entries 0 / 1 only, the remaining wild ones, then the rest in a seeded permutation.  So every batch holds a
        # wild syndrome, every batch of two or more is mixed, every batch of three or more holds entries 2 and 3.
        self.wild = (self.syn > 1).any(axis=1)
        wild = [int(i) for i in np.nonzero(self.wild)[0]]
        past = np.nonzero((self.its > self.T) & (self.conv == 0) & ~self.wild)[0]
        done = np.nonzero(self.conv == 1)[0]
        head = wild[:1] + [int(i) for i in done[:1]] + wild[1:2] + [int(i) for i in past[:1]] + wild[2:]
        rest = [int(i) for i in np.random.default_rng(len(self.syn)).permutation(len(self.syn)) if i not in head]
        self.order = np.array(head + rest, dtype=np.int64)

    def batch(self, B, seed=None):
        """Pool indices of a batch of B: the order above, repeated; with a seed, shuffled."""
        idx = self.order[np.arange(B) % len(self.order)]
        return idx if seed is None else np.random.default_rng(seed).permutation(idx)

    def decoder(self, ldpc):
        return ldpc.BPOTSDecoder(self.H, self.per, self.iters, T=self.T, C=self.C)


def with_wild_entries(syn, seed):
    """A few syndrome entries of 2 and 3 (non-zero flips the sign, :195; > 1 can never be matched, :273), in rows of the
    second half so that the first half stays decodable."""
    syn = syn.copy()
    rng = np.random.default_rng(seed)
    B, s = syn.shape
    for k, v in enumerate((2, 3, 2)):      # (rows B / 2, B / 2 + 1, B / 2 + 2: Pool.order leads with them, 2 before 3)
        syn[B // 2 + (k % max(1, B - B // 2)), int(rng.integers(0, s))] = v
    return syn


# ---- the table of tile widths: (3,6)-regular n -> (S, budget KiB, error rate of the sampled errors = the decoder's per,
#      max_iters, T).  The rates sit above the code's threshold for these lengths and iteration counts, so a pool holds
#      converged and unconverged syndromes (asserted where the pool is used).
WIDTHS = {
    18: (64, 76, 0.10, 12, 3),
    36: (32, 76, 0.10, 12, 3),
    60: (16, 76, 0.09, 12, 3),
    120: (8, 76, 0.08, 12, 3),
    240: (4, 76, 0.07, 12, 2),
    360: (2, 76, 0.07, 12, 2),
    504: (1, 76, 0.07, 12, 2),
    606: (1, 76, 0.07, 12, 2),     # the last n whose S = 1 state fits 76 KiB
    612: (1, 156, 0.07, 12, 2),    # the first that takes the 156 KiB budget
    1200: (1, 156, 0.065, 12, 2),
}
POOL = 48


@functools.lru_cache(maxsize=None)
def width_pool(n, iters=None, T=None):
    ldpc = _ldpc()
    _, _, rate, it0, T0 = WIDTHS[n]
    H = ldpc.codes.parity_check_csc(n, 6, 3)
    E = ldpc.codes.random_errors(n, POOL, rate, seed=1000 + n)
    E[: POOL // 4] &= ldpc.codes.random_errors(n, POOL // 4, 0.5, seed=n)    # a lighter quarter: some converge fast
    syn = with_wild_entries(ldpc.codes.syndromes_of(H, E), n)
    return Pool(H, rate, iters or it0, T or T0, 2.0, syn)


@functools.lru_cache(maxsize=None)
def regular_pool(n, count, rate, iters, T):
    """(3,6)-regular n, `count` syndromes of errors at `rate`: the kernel boundaries by size."""
    ldpc = _ldpc()
    H = ldpc.codes.parity_check_csc(n, 6, 3)
    E = ldpc.codes.random_errors(n, count, rate, seed=n + count)
    E[: count // 3] &= ldpc.codes.random_errors(n, count // 3, 0.6, seed=n)
    return Pool(H, rate, iters, T, 2.0, ldpc.codes.syndromes_of(H, E))


# ---- degree buckets ------------------------------------------------------------------------------------------------------
def widened(n, d, e):
    """parity_check_csc(n, 6, 3) with check 1 widened to exactly d edges (d >= 8) and, independently, bit n - 2 widened to
    exactly e edges (e >= 4); no other check ends above 7 edges and no other bit above 4.  -> (H dense u8, check, bit)."""
    ldpc = _ldpc()
    H = np.asarray(ldpc.codes.parity_check_csc(n, 6, 3).todense()).astype(np.uint8)
    chk, bit = 1, n - 2
    rows = [i for i in range(H.shape[0]) if i != chk and not H[i, bit]]
    H[rows[: e - int(H[:, bit].sum())], bit] = 1                 # other checks: 6 -> 7
    cols = [j for j in range(n) if j != bit and not H[chk, j] and H[:, j].sum() == 3]
    H[chk, cols[: d - int(H[chk].sum())]] = 1                   # other bits: 3 -> 4
    assert H[chk].sum() == d and H[:, bit].sum() == e
    assert H.sum(axis=1).max() == max(d, 7) and H.sum(axis=0).max() == max(e, 4)
    return H, chk, bit


def without_last_edge(H, chk=None, bit=None):
    """H without the last edge of a check (its highest bit: the end of its CSR row) or of a bit (its highest check)."""
    G = H.copy()
    if chk is not None:
        G[chk, np.nonzero(G[chk])[0][-1]] = 0
    else:
        G[np.nonzero(G[:, bit])[0][-1], bit] = 0
    return G


BUCKET_PAIRS = [(8, 4), (9, 4), (32, 4), (8, 5), (8, 16), (9, 5), (32, 16)]     # (d, e) -> <DC, DV>: see bucket_of
WIDE_PAIRS = [(33, 4), (8, 17)]
BUCKET_PER, BUCKET_ITERS, BUCKET_T, BUCKET_B = 0.05, 10, 2, 40


def bucket_of(d, e):
    return (8 if d <= 8 else 32, 4 if e <= 4 else 16)


@functools.lru_cache(maxsize=None)
def bucket_pool(n, d, e):
    ldpc = _ldpc()
    H, chk, bit = widened(n, d, e)
    E = ldpc.codes.random_errors(n, BUCKET_B, BUCKET_PER, seed=100 * d + e)
    E[:, bit] |= (np.arange(BUCKET_B) % 3 == 0).astype(np.uint8)      # the heavy bit is in error in a third of the rows
    syn = ldpc.codes.syndromes_of(H, E)
    return Pool(H, BUCKET_PER, BUCKET_ITERS, BUCKET_T, 2.0, syn), chk, bit


# ---- parameters ----------------------------------------------------------------------------------------------------------
PARAM_PERS, PARAM_ITERS, PARAM_CS = (1e-6, 0.75, 0.9, 1.0), 8, (0.0, 2.0)
PARAM_TS = (1, PARAM_ITERS + 5)


def param_graphs():
    """{name: (H, syndromes)}: a small irregular graph with an empty check and an empty bit, and BB-72."""
    ldpc = _ldpc()
    rng = np.random.default_rng(77)
    H = (rng.random((12, 24)) < 0.2).astype(np.uint8)
    H[4, :] = 0
    H[:, 7] = 0
    syn = rng.integers(0, 2, (70, 12)).astype(np.uint8)
    syn[:20] = (rng.integers(0, 2, (20, 24)).astype(int) @ H.T.astype(int) % 2).astype(np.uint8)
    syn[0] = 0
    syn[33, 2] = 2
    syn[34, 9] = 3
    HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    sx = ldpc.codes.syndromes_of(HX, ldpc.codes.random_errors(72, 40, 0.06, seed=5))
    sx[0] = 0
    sx[21, 5] = 2
    return {"irregular": (H, syn), "bb72": (np.asarray(HX).astype(np.uint8), sx)}


def param_cases():
    return [(per, T, C) for per in PARAM_PERS for T in PARAM_TS for C in PARAM_CS]


@functools.lru_cache(maxsize=None)
def param_pool(name, per, T, C):
    H, syn = param_graphs()[name]
    return Pool(H, per, PARAM_ITERS, T, C, syn)
