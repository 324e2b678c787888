"""Pinned record forms, zeros and ties of the stabilizer min-sum kernel (stab_kernels.hpp) against the numpy model of its rule
(tests/stab_model.py): equality in every element, the LLRs as bit patterns, no tolerance.  The kernel has its own copies of
the record update (the masks around `d0 == 32` and `deg == 64`, the high sign word), of the per-edge second pass that re-runs
`edge()` and restores `hard`, and of the old-message choice `k == oa ? o2 : o1` in two loops -- each with an `edge()` whose
operands are selected by the type of the edge, which changes from edge to edge along every wide check here.  Every case
asserts ON THE MODEL or on the priors alone, before the GPU is touched, that its input gets to the path it is there for
(tests/test_stab_boundaries_cpu.py runs the same assertions without a GPU), asserts the tier, the width and the grid that
ran, and pre-fills its output buffers.

  1  record forms: one graph with checks of degree 31, 32, 33, 63, 64 and 65, types cycling X, Y, Z; the first-sweep minimum
     at the last position alone, the last position and position 31 negative, their written sign set in some columns only;
     alpha 0.75 and 1.0 at a loose clip, and every first-sweep value of the wide checks clamped; batch 65 on both tiers.
     Some column converges before max_iters with the entry of the degree-65 check set: there a lost `hard = tested` would
     turn a matched check into an unmatched one.
  2  zeros and ties of `pauli_decide`: isolated qubits whose prior tables hold every two-way tie (the third belief lower and
     higher), the three-way tie at a negative value, at exactly 0 and at a positive value, and single minima of exactly 0;
     the expected letters are written out.  A connected part has qubits with a prior of exactly 0: the first-sweep m1 is 0
     and the messages are +0 and -0."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from pauli_model import pauli_priors
from stab_model import TX, TY, TZ, StabMinSumModel, symplectic_syndromes
from test_gpu_family_boundaries import DEGREES, B, first_sweep_preconditions
from test_gpu_pauli import frozen, same, tiles_of
from test_gpu_stab import device_entry, host_entry, mixed

pytestmark = pytest.mark.gpu
F = np.float32
N, R, MAX_ITERS = 300, 30, 25
CYCLE = (TX, TY, TZ)                       # the type of position k of a wide check is CYCLE[k % 3]
WIDE = {2: (0, 31), 3: (31, 32), 4: (63, 33), 5: (96, 63), 6: (159, 64), 7: (223, 65)}    # check: (first qubit, degree)
# where the negative prior of a qubit goes so that the edge of that type reads it in u (the header's rule): an X-type edge
# has u = min(GY, GZ) and w from GX, a Z-type edge u = min(GY, GX) and w from GZ, a Y-type edge u = min(GX, GZ) and w from GY.
# The last position takes the second operand of u, position 31 the first.
U_TABLES = {TX: (1, 2), TZ: (1, 0), TY: (0, 2)}      # indices into (prior_x, prior_y, prior_z)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.int32)


@functools.lru_cache(maxsize=None)
def stab_edges():
    """-> (Sx, Sz, probs, s).  30 checks x 300 qubits: check 0 empty, check 1 of degree 1 (qubit 296, Y-type), checks 2 ... 7
    the wide ones on the consecutive qubits 0 ... 287 with types cycling X, Y, Z along the row, 22 random checks of degree
    3 ... 6 over the qubits 0 ... 297 with drawn types; qubit 298 sits in check 8 only, qubit 299 in no check (Y likelier
    than I).  Per-qubit probabilities made from wanted prior tables: every prior in (0.9, 4) except, per wide check i, one
    table of its last qubit = -0.04 i and one of its qubit at position 31 (degree > 32) = -0.5 -- the table that the type
    of that edge reads in u.  65 syndromes: 40 of sampled errors, 25 arbitrary.  The rows do not commute."""
    rng = np.random.default_rng(61)
    T = np.zeros((R, N), dtype=np.int64)
    T[1, 296] = TY
    for i, (first, deg) in WIDE.items():
        T[i, first:first + deg] = [CYCLE[k % 3] for k in range(deg)]
    for i in range(8, R):
        where = rng.choice(298, size=int(rng.integers(3, 7)), replace=False)
        T[i, where] = rng.choice(CYCLE, size=where.size)
    T[8, 298] = TZ
    deg = (T != 0).sum(axis=1)
    assert deg[0] == 0 and deg[1] == 1 and [int(deg[i]) for i in WIDE] == list(DEGREES) and deg[8:].max() <= 7
    assert (T[:, 298] != 0).sum() == 1 and (T[:, 299] != 0).sum() == 0
    assert all({TX, TY, TZ} == set(T[i][T[i] != 0].tolist()) for i in WIDE)
    llr = rng.uniform(0.9, 4.0, size=(3, N))                                # wanted prior_x, prior_y, prior_z
    for i, (first, dg) in WIDE.items():
        last = first + dg - 1
        llr[U_TABLES[int(T[i, last])][1], last] = -0.04 * i
        if dg > 32:
            llr[U_TABLES[int(T[i, first + 31])][0], first + 31] = -0.5
    llr[:, 299] = [2.0, -0.7, 1.5]
    rest = 1.0 / (1.0 + np.exp(-llr).sum(axis=0))
    probs = np.ascontiguousarray((rest[None, :] * np.exp(-llr)).T)         # [n][3]
    Sx, Sz = sp.csc_matrix((T & 1).astype(np.uint8)), sp.csc_matrix((T >> 1).astype(np.uint8))
    ex, ez = ((rng.random((B, N)) < 0.02).astype(np.uint8) for _ in range(2))
    s = symplectic_syndromes(Sx, Sz, ex, ez)
    s[40:] = rng.integers(0, 2, size=(25, R))
    frozen(probs, s)
    return Sx, Sz, probs, s


def stab_first_sweep(priors, rows, types, clip):
    """b_k of every check in sweep 1, from the prior tables and the edge types alone: MX = MY = MZ = +0 and every message
    +0, so GW = prior_W and b_k = clamp((u_k - 0) - w_k) with, by the header's rule, X-type: u = min(GY, GZ), w from GX;
    Z-type: u = min(GY, GX), w from GZ; Y-type: u = min(GX, GZ), w from GY; min(x, y) = x < y ? x : y,
    w = own < 0 ? own : +0.  rows, types: per check the qubits (ascending) and the types of its edges."""
    px, py, pz = (np.asarray(t, dtype=F) for t in priors)
    out = []
    for r, ty in zip(rows, types):
        r, ty = np.asarray(r, dtype=np.int64), np.asarray(ty, dtype=np.int64)
        first = np.where(ty == TY, px[r], py[r])
        second = np.where(ty == TZ, px[r], pz[r])
        own = np.where(ty == TX, px[r], np.where(ty == TZ, pz[r], py[r]))
        u = np.where(first < second, first, second)
        w = np.where(own < 0, own, F(0.0))
        b = np.minimum(np.maximum((u - F(0.0)) - w, -F(clip)), F(clip))
        assert b.dtype == F
        out.append(b)
    return out


def graph_of(Sx, Sz):
    """(rows, types) of the union graph as the model builds them."""
    m = StabMinSumModel(Sx, Sz, np.ones((3, Sx.shape[1]), dtype=F), 1)
    return m.rows, m.types


def wide_first_sweep(clip):
    Sx, Sz, probs, _ = stab_edges()
    rows, types = graph_of(Sx, Sz)
    b = stab_first_sweep(pauli_priors(probs), rows, types, clip)
    return {i: b[i] for i in WIDE}


def stab_edges_reach_their_paths():
    """The preconditions of the fixture, from the priors and the types alone."""
    Sx, Sz, probs, s = stab_edges()
    rows, types = graph_of(Sx, Sz)
    priors = pauli_priors(probs)
    assert (priors < 0).sum() == 6 + 4 + 1                                       # the wide checks' ten and prior_y of qubit 299
    for i, (first, deg) in WIDE.items():
        assert rows[i].tolist() == list(range(first, first + deg)) and types[i].tolist() == [CYCLE[k % 3] for k in range(deg)]
        b = wide_first_sweep(1e6)[i]
        assert len(b) == deg
        first_sweep_preconditions(b, s[:, i], f"check {i} of degree {deg}")


def clamp_clip():
    """Half the smallest nonzero first-sweep |b| of the wide checks."""
    mag = np.abs(np.concatenate(list(wide_first_sweep(1e6).values())))
    clip = float(F(0.5) * mag[mag > 0].min())
    assert 0 < clip < mag[mag > 0].min()
    return clip


@functools.lru_cache(maxsize=None)
def stab_edges_want(alpha, clip):
    Sx, Sz, probs, s = stab_edges()
    want = StabMinSumModel(Sx, Sz, pauli_priors(probs), MAX_ITERS, alpha=alpha, clip=clip).decode(s)
    frozen(*want)
    return want


def record_preconditions(alpha, clamped):
    """Every precondition of a record-form case, on the priors and on the model's outputs alone."""
    Sx, Sz, probs, s = stab_edges()
    stab_edges_reach_their_paths()
    clip = clamp_clip() if clamped else 1e6
    want = stab_edges_want(alpha, clip)
    gx, gz, conv, its, G = want
    if clamped:
        for i, b in wide_first_sweep(clip).items():
            assert (np.abs(b) == F(clip)).all(), f"check {i}: an edge is not clamped"
            assert (b < 0).sum() == (2 if len(b) > 32 else 1) and b[-1] < 0      # the signs are what is left
        loose = stab_edges_want(alpha, 1e6)
        assert (bits(G) != bits(loose[4])).any(axis=(1, 2)).all(), "the clamp leaves a column as it was"
        # a message is at most alpha * clip = 0.03 against priors of 0.9 and more: hardly a decision moves, and the decision
        # of the priors matches none of the 65 syndromes -- every column runs all sweeps, the records are rewritten 25
        # times, and what can differ is the signs (the convergence preconditions below are those of the loose cases)
        assert not conv.any() and (its == MAX_ITERS).all() and (gx[:, 299] & gz[:, 299]).all()
        return want
    mixed(conv, B)
    assert len(set(its.tolist())) >= 3, sorted(set(its.tolist()))
    assert (gx[:, 299] & gz[:, 299]).all()                                 # the qubit in no check is a Y in every column
    early = (conv == 1) & (its < MAX_ITERS) & (s[:, 7] != 0)
    assert early.any(), "no column converges before max_iters with the entry of the degree-65 check set"
    return want


CASES = [(0.75, False), (1.0, False), (0.75, True)]


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("alpha, clamped", CASES)
def test_stab_record_forms_at_degrees_31_to_65(ldpc, gpu, alpha, clamped, variant):
    """The four-word record with the mask `(1u << d0) - 1u` at degree 31 and `d0 == 32` at 32; five words with
    `(1u << (deg - 32)) - 1u` at 33 and 63 and `deg == 64` at 64, the old minimum position in the `k >= 32` loop; a word per
    edge with the second `edge()` pass and `hard = tested` at 65.  The clamped case leaves every first-sweep |b| of the wide
    checks at clip: `a` stays kMsNone and the records hold alpha * clip twice."""
    Sx, Sz, probs, s = stab_edges()
    want = record_preconditions(alpha, clamped)
    clip = clamp_clip() if clamped else 1e6
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, None, MAX_ITERS, alpha=alpha, clip=clip, pauli_probs=probs, kernel_variant=variant,
                                       check=False)
    assert all(np.array_equal(bits(got), bits(p)) for got, p in zip((dec.prior_x, dec.prior_y, dec.prior_z), pauli_priors(probs)))
    S = dec.tile_syndromes
    assert (dec.kernel, dec.last_grid) == (variant, 0) and 1 <= S <= 64 and (dec.n, dec.rows) == (N, R)
    what = f"record forms alpha {alpha} clip {clip}, tier {variant}"
    same(device_entry(dec, s), want, what + ", device entry")
    assert dec.last_grid == tiles_of(B, S) >= 2
    same(host_entry(dec, s), want, what + ", host entry")
    assert dec.last_grid == tiles_of(B, S)
    dec.close()


# ---- 2. zeros and ties -------------------------------------------------------------------------------------------------------
# (px, py, pz) of an isolated qubit, the Pauli the rule decides, and why.  A belief is log(pI / pW): the LOWER belief is the
# likelier Pauli, a tie of equal probabilities is a tie of equal bit patterns (one division and one log of the same numbers),
# and pI == pW in binary fractions is a belief of exactly +0.  The rule: best = X, g = GX; Z only if GZ < g; Y only if
# GY < g; the Pauli only if g <= 0.
TIES = [
    ((0.35, 0.05, 0.35), "X", "GX == GZ < 0 < GY: the tie keeps X"),
    ((0.25, 0.40, 0.25), "Y", "GY < GX == GZ < 0: the third belief is lower"),
    ((0.35, 0.35, 0.05), "X", "GX == GY < 0 < GZ: the tie keeps X"),
    ((0.25, 0.25, 0.40), "Z", "GZ < GX == GY < 0"),
    ((0.05, 0.35, 0.35), "Z", "GY == GZ < 0 < GX: Z comes before Y"),
    ((0.40, 0.25, 0.25), "X", "GX < GY == GZ < 0"),
    ((0.30, 0.30, 0.30), "X", "the three-way tie at a negative value"),
    ((0.25, 0.25, 0.25), "X", "the three-way tie at exactly 0: g <= 0"),
    ((0.10, 0.10, 0.10), "I", "the three-way tie at a positive value"),
    ((0.375, 0.125, 0.125), "X", "a single minimum of exactly 0 in GX"),
    ((0.125, 0.375, 0.125), "Y", "a single minimum of exactly 0 in GY"),
    ((0.125, 0.125, 0.375), "Z", "a single minimum of exactly 0 in GZ"),
    ((0.3125, 0.0625, 0.3125), "X", "GX == GZ == 0 < GY"),
    ((0.0625, 0.3125, 0.3125), "Z", "GY == GZ == 0 < GX"),
    ((0.3125, 0.3125, 0.0625), "X", "GX == GY == 0 < GZ"),
    ((0.01, 0.02, 0.03), "I", "no tie, every belief positive"),
]
TIE_LETTERS = "XYXZZXXXIXYZXZXI"
ZERO_PRIOR = {"X": (0.375, 0.125, 0.125), "Y": (0.125, 0.375, 0.125), "Z": (0.125, 0.125, 0.375)}     # prior_W == +0, the others log 3
# the connected part: 4 checks over the qubits 16 ... 22; qubit 16 has prior_z == 0 and sits on an X-type edge (u = min(GY, GZ)
# = 0) and a Y-type edge (u = min(GX, GZ) = 0), qubit 19 has prior_x == 0 on a Z-type and a Y-type edge, qubit 21 has prior_y == 0
# on an X-type edge: the first-sweep m1 of every check is 0, in check 1 (two such edges) m2 as well
TIE_CHECKS = ["XZYIIII", "YIIZXII", "IXIYZII", "IIZIIXY"]
TIE_ZEROS = {16: "Z", 19: "X", 21: "Y"}
TIE_N, TIE_ITERS = len(TIES) + 7, 6


@functools.lru_cache(maxsize=None)
def ties_case():
    """-> (Sx, Sz, probs, s, model output, the model's last messages).  16 isolated qubits with the tables of TIES, then the
    connected part; all 16 syndromes of the 4 checks."""
    T = np.zeros((4, TIE_N), dtype=np.int64)
    for i, row in enumerate(TIE_CHECKS):
        assert len(row) == 7
        T[i, len(TIES):] = [{"I": 0, "X": TX, "Y": TY, "Z": TZ}[c] for c in row]
    Sx, Sz = sp.csc_matrix((T & 1).astype(np.uint8)), sp.csc_matrix((T >> 1).astype(np.uint8))
    probs = np.random.default_rng(3).uniform(0.02, 0.09, (TIE_N, 3))
    probs[:len(TIES)] = [p for p, _, _ in TIES]
    for j, letter in TIE_ZEROS.items():
        probs[j] = ZERO_PRIOR[letter]
    s = ((np.arange(16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    model = StabMinSumModel(Sx, Sz, pauli_priors(probs), TIE_ITERS)
    want = model.decode(s)
    messages = [np.array(c) for c in model.last_messages]
    frozen(probs, s, *want, *messages)
    return Sx, Sz, probs, s, want, messages


def tie_tables_are_exact(prior_x, prior_y, prior_z):
    """On three prior tables as bit patterns: the ties are equal words, the zeros are +0, the order of the rest is TIES'."""
    P = np.stack([bits(prior_x), bits(prior_y), bits(prior_z)])
    V = np.stack([np.asarray(t, dtype=F) for t in (prior_x, prior_y, prior_z)])
    k = {"X": 0, "Y": 1, "Z": 2}
    for j, pair, third in ((0, "XZ", "Y"), (1, "XZ", "Y"), (2, "XY", "Z"), (3, "XY", "Z"), (4, "YZ", "X"), (5, "YZ", "X")):
        a, b, c = k[pair[0]], k[pair[1]], k[third]
        assert P[a, j] == P[b, j] and V[a, j] < 0, f"qubit {j}: no tie of {pair} at a negative value"
        assert (V[c, j] > 0) if j % 2 == 0 else (V[c, j] < V[a, j]), f"qubit {j}: the third belief is on the wrong side"
    assert P[0, 6] == P[1, 6] == P[2, 6] and V[0, 6] < 0
    assert P[0, 7] == P[1, 7] == P[2, 7] == 0                               # +0: the word 0, not 0x80000000
    assert P[0, 8] == P[1, 8] == P[2, 8] and V[0, 8] > 0
    for j, w in ((9, 0), (10, 1), (11, 2)):
        assert P[w, j] == 0 and all(V[o, j] > 0 for o in range(3) if o != w)
    for j, pair, third in ((12, "XZ", "Y"), (13, "YZ", "X"), (14, "XY", "Z")):
        assert P[k[pair[0]], j] == P[k[pair[1]], j] == 0 and V[k[third], j] > 0
    assert (V[:, 15] > 0).all()
    for j, letter in TIE_ZEROS.items():
        assert P[k[letter], j] == 0 and all(V[o, j] > 0 for o in range(3) if o != k[letter])


def ties_preconditions():
    """On the model and the priors alone.  -> the model output."""
    Sx, Sz, probs, s, want, messages = ties_case()
    priors = pauli_priors(probs)
    tie_tables_are_exact(*priors)
    gx, gz, conv, its, G = want
    assert "".join(letter for _, letter, _ in TIES) == TIE_LETTERS
    # an isolated qubit keeps its prior (the totals are +0) and its decision in every column: the letters, as literals
    assert (bits(G[:, :, :len(TIES)]) == bits(priors[:, :len(TIES)])[None]).all()
    decided = np.array(list("IXZY"))[gx[:, :len(TIES)] + 2 * gz[:, :len(TIES)]]
    assert all("".join(row) == TIE_LETTERS for row in decided), ["".join(row) for row in decided][:2]
    ex, ez = StabMinSumModel._decide(*(np.asarray(t, dtype=F)[None, :len(TIES)] for t in priors))
    assert "".join(np.array(list("IXZY"))[ex[0] + 2 * ez[0]]) == TIE_LETTERS          # _decide on the tables alone
    # the connected part: the first-sweep b of a zero-prior qubit is +0 on the edges that read the zero in u, so m1 == 0
    rows, types = graph_of(Sx, Sz)
    b1 = stab_first_sweep(priors, rows, types, 1e6)
    assert [int((bits(b) == 0).sum()) for b in b1] == [1, 2, 1, 1] and all((b >= 0).all() for b in b1)      # +0, never -0
    # ... and messages of both zeros are there at the end, in converged and in unconverged columns
    words = np.concatenate([bits(c).ravel() for c in messages])
    assert (words == 0).any() and (words == np.int32(-2 ** 31)).any(), "no +0 or no -0 message at the end"
    minus = np.array([(bits(c) == np.int32(-2 ** 31)).any(axis=1) for c in messages]).any(axis=0)     # [column]
    assert minus.any()
    mixed(conv, 16)
    return want


@pytest.mark.parametrize("variant", [1, 2])
def test_stab_zeros_and_ties_of_the_decision(ldpc, gpu, variant):
    """`pauli_decide`: X, then Z only if `gz < g`, then Y only if `gy < g`, the Pauli only if `g <= 0` -- on tables that tie
    exactly and on beliefs of exactly 0, with the letters written out; and messages of +0 and -0 from checks whose first-sweep
    m1 is 0.  The LLR planes are compared as bit patterns, the sign of a zero included."""
    Sx, Sz, probs, s, _, _ = ties_case()
    want = ties_preconditions()
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, None, TIE_ITERS, pauli_probs=probs, kernel_variant=variant, check=False)
    tie_tables_are_exact(dec.prior_x, dec.prior_y, dec.prior_z)
    assert all(np.array_equal(bits(got), bits(p)) for got, p in zip((dec.prior_x, dec.prior_y, dec.prior_z), pauli_priors(probs)))
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (variant, 64, 0)
    what = f"zeros and ties, tier {variant}"
    got = device_entry(dec, s)
    assert dec.last_grid == 1
    decided = np.array(list("IXZY"))[got[0][:, :len(TIES)] + 2 * got[1][:, :len(TIES)]]
    assert all("".join(row) == TIE_LETTERS for row in decided), (what, ["".join(row) for row in decided][:2])
    same(got, want, what + ", device entry")
    same(host_entry(dec, s), want, what + ", host entry")
    dec.close()
