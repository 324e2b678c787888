"""Pinned boundary shapes of the bit-flip, min-sum, relay and device OSD kernels against their numpy models
(tests/bitflip_model.py, minsum_model.py, relay_model.py, osd_model.py): equality in every element, for min-sum and relay
including the LLR bit patterns.  Each case is built to reach one path of a kernel that the other suites do not reach, and
asserts ON THE MODEL, before the GPU is touched, that its input really gets there:

  1  bit-flip rank search with G = ceil(n / 64) > 64 groups, C = ceil(G / 64) of them to a lane (bitflip_kernels.hpp: a
     lane that owns fewer than C groups, lanes that own none, the `g < G - 1` guard with a partial last group)
  2  bit-flip nodes heavier than a wave: bits in 70 and 130 checks, a check of degree 64 (rw_shift 6) and 65 (rw_shift 7)
  3  min-sum / relay record forms at check degrees 31, 32, 63 and 65 with the minimum at the last position and the top
     sign bit of a word set (minsum_kernels.hpp: the masks around d0 == 32 and deg == 64)
  4  device OSD at orders 11, 12 and 16 (kOsdMaxOrder), on a rank-deficient matrix and on one with two row blocks"""
import numpy as np
import pytest
import scipy.sparse as sp

from bitflip_model import TIE_FIRST, TIE_LAST, TIE_RANDOM, BitFlipModel, chooser_for
from minsum_model import MinSumModel, llr_of_probs
from osd_model import osd_model_postprocess
from relay_model import RelayModel
from test_gpu_bitflip import _assert_equal_to_model
from test_gpu_minsum import _device as _ms_device
from test_gpu_minsum import _same as _ms_same
from test_gpu_osd_device import _device as _osd_device
from test_gpu_osd_device import _syn_of
from test_gpu_relay import _both_entries as _rl_both_entries
from test_gpu_relay import _decoder as _rl_decoder
from test_gpu_relay import _gammas

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5
RULES = (("random", TIE_RANDOM), ("first", TIE_FIRST), ("last", TIE_LAST))


# ---- bit-flip ----------------------------------------------------------------------------------------------------------
def _bitflip_model_with_trace(H, syn, max_iters, tie, seed):
    """-> ((err, conv, iters, stop) as decode_batch gives them, the flipped bits of every column in one list)."""
    model = BitFlipModel(H, max_iters)
    ch = chooser_for(tie, seed)
    B = syn.shape[0]
    err = np.zeros((B, model.n), dtype=np.uint8)
    conv, its, stop = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    flipped = []
    for i in range(B):
        trace = []
        err[i], c, its[i], stop[i] = model.decode(syn[i], ch, column=i, trace=trace)
        conv[i] = c
        flipped += [(i, int(step[3])) for step in trace]
    return (err, conv, its, stop), flipped


def _bitflip_on_every_tier(ldpc, H, syn, max_iters, rule, seed, want, variants, must_run):
    ran = []
    for variant in variants:
        try:
            dec = ldpc.BitFlipDecoder(H, 0.01, max_iters, tie_break=rule, seed=seed, kernel_variant=variant)
        except ldpc.LdpcError as e:
            assert variant not in must_run and variant in (1, 2) and e.status == UNSUPPORTED, (variant, e)
            continue
        assert dec.kernel == (variant or dec.kernel) and dec.kernel in (1, 2, 3)
        _assert_equal_to_model(dec.decode_batch_host(syn, column0=0), want, f"{rule}, kernel_variant {variant} (tier {dec.kernel})")
        ran.append(variant)
        dec.close()
    assert set(must_run) <= set(ran), (ran, must_run)
    return ran


@pytest.mark.parametrize("n,G,C", [(4100, 65, 2), (8200, 129, 3)])
def test_bitflip_rank_search_with_more_than_64_groups_and_a_partial_last_one(ldpc, gpu, n, G, C):
    """n = 4100: G = 65, C = 2 -- lane 32 owns one group, lanes 33 ... 63 none, the last group has 4 bits.  n = 8200:
    G = 129, C = 3 -- lane 42 owns the groups 126 ... 128, lanes 43 ... 63 none, the last group has 8 bits."""
    assert ((n + 63) // 64, (G + 63) // 64) == (G, C) and n % 64 != 0 and G < 64 * C   # a partial last group, lanes without a group
    H = ldpc.codes.parity_check_csc(n, 10, 5)
    rng = np.random.default_rng(1)
    B = 24
    E = np.zeros((B, n), dtype=np.uint8)
    for b in range(B):   # 2 of the last 4 bits and 6 others
        E[b, n - 4 + rng.choice(4, size=2, replace=False)] = 1
        E[b, rng.choice(n - 4, size=6, replace=False)] = 1
    syn = ldpc.codes.syndromes_of(H, E)
    for rule, tie in RULES:
        want, flipped = _bitflip_model_with_trace(H, syn, 30, tie, seed=3)
        groups = np.array([j // 64 for _, j in flipped])
        in_last = int((groups == G - 1).sum())
        print(f"n {n} {rule}: {len(flipped)} flips, {in_last} in the last group, {int((groups % C != 0).sum())} in a group g with g % C != 0")
        assert in_last > 0, "no flip lands in the last (partial) group"
        assert (groups % C != 0).any(), "no flip lands in a group that is not the first of its lane"
        ran = _bitflip_on_every_tier(ldpc, H, syn, 30, rule, 3, want, (0, 1, 2, 3), must_run=(0, 3))
        assert 1 not in ran      # n > 2048: the one-wave tier does not take it


def _heavy_graph(cdeg, seed):
    """140 checks x 200 bits: bit 0 in 70 checks, bit 1 in 130, check 0 of degree `cdeg` (the largest: bits 0 ... cdeg - 1),
    the other bits of degree 2 ... 4, check 139 and bit 199 empty."""
    rng = np.random.default_rng(seed)
    s, n = 140, 200
    A = np.zeros((s, n), dtype=np.uint8)
    A[0, :cdeg] = 1
    A[1 + rng.choice(s - 2, size=69, replace=False), 0] = 1
    A[1 + rng.choice(s - 2, size=129, replace=False), 1] = 1
    for j in range(2, n - 1):
        d = int(rng.integers(2, 5)) - int(A[0, j])
        A[1 + rng.choice(s - 2, size=d, replace=False), j] = 1
    cd, bd = A.sum(axis=1), A.sum(axis=0)
    assert bd[0] == 70 and bd[1] == 130 and bd[n - 1] == 0 and cd[s - 1] == 0
    assert cd[0] == cdeg and cd[1:].max() < cdeg and 2 <= bd[2:n - 1].min() and bd[2:n - 1].max() <= 4
    return sp.csc_matrix(A)


@pytest.mark.parametrize("cdeg,rw_shift", [(64, 6), (65, 7)])
def test_bitflip_bits_in_more_checks_than_a_wave_has_lanes(ldpc, gpu, cdeg, rw_shift):
    """The flip loop of the one-wave tier takes two and three rounds (70 and 130 checks over 64 threads), and the
    (check, bit) pairs of a flip number deg << rw_shift = 130 << 7 = 16,640."""
    H = _heavy_graph(cdeg, seed=cdeg)
    shift = 0
    while (1 << shift) < cdeg:      # the host's rule for rw_shift (ldpc_bitflip.hip)
        shift += 1
    assert shift == rw_shift
    rng = np.random.default_rng(100 + cdeg)
    B = 65
    E = (rng.random((B, 200)) < 0.02).astype(np.uint8)
    E[:, 0] = np.arange(B) % 3 != 1          # the heavy bits: one, the other or both
    E[:, 1] = np.arange(B) % 3 != 0
    syn = ldpc.codes.syndromes_of(H, E)
    for rule, tie in RULES:
        want, flipped = _bitflip_model_with_trace(H, syn, 30, tie, seed=11)
        bits = {j for _, j in flipped}
        assert 0 in bits and 1 in bits, f"{rule}: a heavy bit is never flipped"
        assert len(set(want[3].tolist())) >= 2, "one stop reason only"
        _bitflip_on_every_tier(ldpc, H, syn, 30, rule, 11, want, (1, 2, 3), must_run=(1, 2, 3))


# ---- min-sum and relay -------------------------------------------------------------------------------------------------
EDGE_CHECKS = {2: (0, 31), 3: (31, 32), 4: (63, 63), 5: (126, 65)}    # check: (first bit, degree) -- consecutive bits


@pytest.fixture(scope="module")
def record_edges():
    """30 checks x 200 bits: check 0 empty, check 1 of degree 1, checks 2 / 3 / 4 / 5 of degree 31 / 32 / 63 / 65 on the
    consecutive bits 0 ... 190, 24 random checks of degree 3 ... 6 over the bits 0 ... 197; bit 198 sits in check 6 only,
    bit 199 in none (negative prior).  In each of the four checks the LAST bit has the smallest |prior| and a negative
    prior, and where the check has one, so has its bit at position 31 (with a larger |prior|).  65 syndromes: 40 of
    sampled errors, 25 arbitrary."""
    rng = np.random.default_rng(31)
    s, n = 30, 200
    Hd = np.zeros((s, n), dtype=np.uint8)
    Hd[1, 193] = 1
    for i, (first, deg) in EDGE_CHECKS.items():
        Hd[i, first:first + deg] = 1
    for i in range(6, s):
        Hd[i, rng.choice(198, size=int(rng.integers(3, 7)), replace=False)] = 1
    Hd[6, 198] = 1
    assert Hd[0].sum() == 0 and Hd[1].sum() == 1 and Hd[:, 198].sum() == 1 and Hd[:, 199].sum() == 0
    assert [int(Hd[i].sum()) for i in (2, 3, 4, 5)] == [31, 32, 63, 65] and Hd[6:].sum(axis=1).max() <= 7
    prior = llr_of_probs(rng.uniform(0.01, 0.3, n))
    assert prior.min() > 0.8
    prior[199] = np.float32(-0.8)
    prior[195] = np.float32(1e-40)       # a subnormal prior (bits 191 ... 197 sit in random checks only)
    prior[196] = np.float32(-0.0)
    for i, (first, deg) in EDGE_CHECKS.items():
        prior[first + deg - 1] = np.float32(-0.05 * i)
        if deg > 32:
            prior[first + 31] = np.float32(-0.5)
    e = (rng.random((65, n)) < 0.03).astype(np.uint8)
    syn = ((Hd.astype(np.int64) @ e.T.astype(np.int64)) % 2).T.astype(np.uint8)
    syn[40:, :] = rng.integers(0, 2, size=(25, s))
    H = sp.csc_matrix(Hd)
    # ---- what the first check sweep writes, from the priors alone: in sweep 1 every message is +0, so b_k is the prior
    # (|prior| < clip), a is the first position of the smallest |b_k|, and edge k is negative iff par ^ neg_k with
    # par = syndrome ^ XOR neg
    for i, (first, deg) in EDGE_CHECKS.items():
        b = prior[first:first + deg]
        mag = np.abs(b)
        assert int(np.argmin(mag)) == deg - 1 and (mag[:-1] > mag[-1]).all(), f"check {i}: the minimum is not at the last position alone"
        neg = b < 0
        assert neg[-1] and neg.sum() == (2 if deg > 32 else 1)
        par = (syn[:, i] != 0) ^ (neg.sum() % 2 == 1)
        sign = par[:, None] ^ neg[None, :]                     # [column][position]
        assert sign[:, deg - 1].any() and not sign[:, deg - 1].all(), f"check {i}: the top sign bit is set in no column / in every column"
        if deg >= 32:                                          # bit 31 of the first sign word
            assert sign[:, 31].any() and not sign[:, 31].all()
    return H, prior, syn


def _tiers(ldpc, make):
    """The decoders of kernel_variant 1 and 2; UNSUPPORTED is acceptable for variant 1 only."""
    out = []
    for variant in (1, 2):
        try:
            dec = make(variant)
        except ldpc.LdpcError as e:
            assert variant == 1 and e.status == UNSUPPORTED, (variant, e)
            continue
        assert dec.kernel == variant
        out.append((variant, dec))
    assert 2 in [v for v, _ in out]
    return out


@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_minsum_record_forms_at_degrees_31_32_63_65(ldpc, gpu, record_edges, alpha):
    H, prior, syn = record_edges
    want = MinSumModel(H, prior, 20, alpha=alpha).decode(syn)
    assert want[1].any() and not want[1].all(), "the model converges on every column or on none"
    assert want[0][:, 199].all()
    for variant, dec in _tiers(ldpc, lambda v: ldpc.MinSumDecoder(H, None, 20, channel_llr=prior, alpha=alpha, kernel_variant=v)):
        assert dec.info().tile_syndromes <= 64      # batch 65: at least one full tile and a ragged one
        _ms_same(_ms_device(dec, syn), want, f"alpha {alpha}, tier {variant}")
        dec.close()


def test_relay_record_forms_at_degrees_31_32_63_65(ldpc, gpu, record_edges):
    H, prior, syn = record_edges
    g = _gammas(3, 200, seed=8)
    legs = [8, 6, 6]
    want = RelayModel(H, prior, g, legs, stop_after=2).decode(syn)
    assert want[1].any() and not want[1].all(), "the model finds a solution for every column or for none"
    assert (want[2] > legs[0]).any(), "no column goes beyond the first leg"
    for variant, dec in _tiers(ldpc, lambda v: _rl_decoder(ldpc, H, prior, g, legs, stop_after=2, kernel_variant=v)):
        _rl_both_entries(dec, syn, want, f"tier {variant}")
        dec.close()


# ---- device OSD --------------------------------------------------------------------------------------------------------
def _gf2_rank(A):
    A = (np.asarray(A) & 1).astype(np.uint8).copy()
    r = 0
    for c in range(A.shape[1]):
        p = np.nonzero(A[r:, c])[0]
        if p.size == 0:
            continue
        A[[r, r + p[0]]] = A[[r + p[0], r]]
        rows = np.nonzero(A[:, c])[0]
        A[rows[rows != r]] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def _osd_inputs(Hd, B, seed):
    """Consistent syndromes (of random errors) with drawn bp_err and LLRs that tie, as test_word_boundaries_in_rows_and_columns draws them."""
    rng = np.random.default_rng(seed)
    n = Hd.shape[1]
    syn = _syn_of(Hd, (rng.random((B, n)) < 0.1).astype(np.uint8))
    err = (rng.random((B, n)) < 0.1).astype(np.uint8)
    llr = -np.exp(rng.uniform(-8, 1, (B, n)))
    llr[rng.random((B, n)) < 0.3] = llr[0, 0]
    return syn, err, llr


def _osd_against_model(ldpc, Hd, order, syn, err, llr, tiers):
    H = sp.csc_matrix(Hd)
    want = np.stack([osd_model_postprocess(Hd, syn[b], err[b], llr[b], order) for b in range(syn.shape[0])])
    assert np.array_equal(_syn_of(Hd, want), syn), "a model output does not reproduce its syndrome"
    for variant, tier in tiers:
        out = _osd_device(ldpc, H, order, syn, err, llr, variant=variant, tier=tier)
        bad = np.nonzero((out != want).any(axis=1))[0]
        assert bad.size == 0, f"order {order} kernel_variant {variant}: syndromes {bad.tolist()} differ from the model"
    return want


@pytest.mark.parametrize("order", [11, 16])
def test_osd_orders_11_and_16_on_a_rank_deficient_matrix(ldpc, gpu, order):
    """24 x 60: row 5 empty, row 9 = row 2 + row 17; the search set has `order` columns (n - rank >= 16), 2^16 candidates
    over the 64 lanes of tier 1 and the 1024 of tiers 2 and 3."""
    rng = np.random.default_rng(24)
    Hd = (rng.random((24, 60)) < 0.15).astype(np.uint8)
    Hd[5, :] = 0
    Hd[9, :] = Hd[2] ^ Hd[17]
    rank = _gf2_rank(Hd)
    assert rank <= 22 and 60 - rank >= 16 and Hd[9].any()
    syn, err, llr = _osd_inputs(Hd, 16, seed=order)
    want = _osd_against_model(ldpc, Hd, order, syn, err, llr, ((0, 1), (2, 2), (3, 3)))
    lower = np.stack([osd_model_postprocess(Hd, syn[b], err[b], llr[b], order - 6) for b in range(4)])
    assert (want[:4] != lower).any(), "the higher order changes no estimate: the candidates beyond 2^(order - 6) never win"


def test_osd_order_12_with_two_row_blocks(ldpc, gpu):
    """70 x 120: a lane of tier 1 owns two rows, and a bitset over the rows (a candidate's pivot bits) has two words."""
    rng = np.random.default_rng(70)
    Hd = (rng.random((70, 120)) < 0.06).astype(np.uint8)
    rank = _gf2_rank(Hd)
    assert 64 < rank and 120 - rank >= 12, rank      # pivots in both row blocks, a search set of 12 columns
    syn, err, llr = _osd_inputs(Hd, 16, seed=12)
    _osd_against_model(ldpc, Hd, 12, syn, err, llr, ((0, 1), (2, 2), (3, 3)))
