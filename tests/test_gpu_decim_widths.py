"""The guided-decimation min-sum kernel (decim_kernels.hpp) at EVERY tile width, under both LDS budgets, with ties that sit in
different threads of a lane, with D at whole words and with SLOT REUSE below S = 64 and in the product build, against the
numpy model of its rule (tests/decim_model.py); and the LARGEST state the planner admits on chip, launched once for each
kernel of the family (plain min-sum, relay, Pauli, decimation) against its model.  Equality in every element -- errors,
flags, iteration counts, decimation counts, and the LLRs as bit patterns; the arithmetic has no division and no
transcendental, so there is no tolerance.

The kernel indexes every row of L, the records, D and the syndromes by `<< sh` with `l = t & (S - 1)`, `q = t >> sh`,
`Q = T >> sh`: at S = 64 a lane is shared by 8 threads of the on-chip kernel, at S = 1 by all 512, and they meet in the one
`atomicMax` on `sh_key[l]` and in the `q == 0` write of the pin.  tests/test_gpu_decim.py runs S = 64 and 16 only.

What ran is read back and asserted (`info().kernel`, `.tile_syndromes`, `.last_grid`), so a case that misses its width or
whose workgroups never take a second tile fails instead of passing on another path, and every case asserts ON THE MODEL,
before anything touches the GPU, that its input holds what it is there for:

  1. every row of DECIM_TABLE (tests/test_decim_cpu.py holds it against the planner): S = 64 ... 1 under 79 KiB, S = 2 and
     S = 1 under 159 KiB, the unlimited tier by size and forced, with per-bit priors and a waterfall across the batch
  2. the tie rule -- the lowest index on a tie -- with a uniform prior at S = 32, 16 and 8 and in the unlimited tier, where
     the tied bits belong to different threads of a lane
  3. D at whole words: n = 32 and 64 (no partial last word), n = 33 (a last word of one bit), every bit free to be pinned
  4. a tile after another in one slot: nine tiles of 16 under a capped grid, more tiles than resident workgroups in the
     product build, and two handles of widths 64 and 1 alive together
  5. a one-syndrome state of exactly 159 KiB, the largest the planner admits, for the four kernels

Model cost.  The models loop over the edges in Python; a decimation model of T (Dmax + 1) iterations costs what a min-sum
model of as many does.  On one CPU core: every row of the table up to n = 768 at most 1.1 s, n = 6432 1.6 s, n = 12288
2.1 s, n = 13824 4.1 s; the four models of section 5 stay below 10 s each.  Every result is computed once and shared."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from decim_model import DecimModel
from minsum_model import MinSumModel, llr_of_probs
from pauli_model import PauliMinSumModel, pauli_priors
from relay_model import RelayModel
from test_decim_cpu import DECIM_TABLE, lib_plan
from test_gpu_decim import _c240, _device, _host, _rows, _same
from test_gpu_minsum_tiles import batch_of, gammas_of, make_decoder, ragged_prefix_of, reuse_preconditions, rows_of, tiles_of, waterfall_inputs
from test_gpu_minsum_tiles import device_entry as family_device
from test_gpu_minsum_tiles import same as family_same
from test_gpu_pauli import device_entry as pauli_device
from test_gpu_pauli import same as pauli_same
from test_tile_plan_cpu import debug_plan

pytestmark = pytest.mark.gpu
F = np.float32
OK, UNSUPPORTED = 0, 5
KIB159 = 159 * 1024


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


def frozen(want):
    for x in want:
        x.setflags(write=False)
    return want


def decoder(ldpc, H, prior, T, Dmax, variant=0):
    return ldpc.DecimatedMinSumDecoder(H, None, T, channel_llr=prior, max_decimations=Dmax, kernel_variant=variant)


def what_ran(dec):
    info = dec.info()
    return info.kernel, info.tile_syndromes, info.last_grid


# ---- 1. every width ---------------------------------------------------------------------------------------------------------
# n of DECIM_TABLE -> (round_iters, max_decimations): fewer of both as the model gets dearer
ROUNDS = {96: (3, 6), 192: (3, 6), 384: (3, 4), 768: (3, 4), 1536: (2, 3), 3072: (2, 3), 6144: (2, 2), 6432: (2, 2),
          12288: (2, 1), 13824: (2, 1)}


@functools.lru_cache(maxsize=None)
def width_case(n, S):
    """The inputs of a table row at tile width S -- per-bit priors, row b sampled at 0.1 ... 1.9 times the bits'
    probabilities -- and the model's output on them.  -> (H, prior, syn, T, Dmax, model output)."""
    B = batch_of(S)
    T, Dmax = ROUNDS[n]
    H, prior, syn = waterfall_inputs(n, B, 0.05)
    err, conv, its, ndec, L = want = frozen(DecimModel(H, prior, T, Dmax).decode(syn))
    # preconditions, on the model alone
    assert 0 < conv.sum() < B, (n, int(conv.sum()), B)
    assert ((conv == 1) & (ndec > 0)).any(), f"n {n}: no row converged after a decimation"
    assert ((conv == 0) & (ndec == Dmax)).any(), f"n {n}: no row gave up with every decimation spent"
    if B >= 10:
        assert set(ndec.tolist()) == set(range(Dmax + 1)), (n, sorted(set(ndec.tolist())))
    if B >= 5:
        assert len(set(its.tolist())) >= 3, (n, sorted(set(its.tolist())))
    return H, prior, syn, T, Dmax, want


@functools.lru_cache(maxsize=None)
def mirrored_case(n, S):
    """Pins of BOTH signs at the row's width.  The waterfall's most reliable bits all have L > 0 (on the inputs above the
    model pins 801 bits over the ten rows and not one of them at -2 clip), so a kernel that wrote every pin as +2 clip would
    pass them.  Here a random half of the bits is mirrored: their priors are negated and their column of H is added to every
    syndrome, as if each of them had been sent flipped -- the most reliable bit of a lane is then as often one with L < 0.
    Rounds of ONE iteration (a decimation after every iteration) keep the second model of a row cheaper than the first.
    -> (prior, syn, T, Dmax, model output)."""
    H, prior, syn, _, Dmax, _ = width_case(n, S)
    rng = np.random.default_rng(n + 1)
    flip = rng.random(n) < 0.5
    mirrored = np.where(flip, -prior, prior).astype(F)
    msyn = syn ^ _ldpc().codes.syndromes_of(H, flip[None, :].astype(np.uint8))
    model = DecimModel(H, mirrored, 1, Dmax)
    err, conv, its, ndec, L = want = frozen(model.decode(msyn))
    D = model.last_D
    assert D.any() and (np.abs(L[D]) == F(2e6)).all() and (L[D] < 0).any() and (L[D] > 0).any(), (n, int((L[D] < 0).sum()), int(D.sum()))
    assert ((conv == 0) & (ndec == Dmax)).any()
    return mirrored, msyn, 1, Dmax, want


@pytest.mark.parametrize("n", sorted(DECIM_TABLE))
def test_every_width_of_the_table_equals_the_model(ldpc, gpu, n):
    """One row of the table, automatic selection: the tier and the width are asserted BEFORE the decode; the whole batch
    (2 S + S / 2 + 5 syndromes) and its prefix of two full tiles and a ragged one go through the device entry, the rows of
    the widest width and of S = 1 and S = 2 where the budgets meet also through the host entry; then the mirrored inputs
    (mirrored_case: pins of both signs) through the device entry."""
    tier, S, _ = DECIM_TABLE[n]
    H, prior, syn, T, Dmax, want = width_case(n, S)
    B = syn.shape[0]
    dec = decoder(ldpc, H, prior, T, Dmax)
    assert what_ran(dec) == (tier, S, 0), (dec.info(), tier, S)
    what = f"decimation n {n} tier {tier} S {S} T {T} Dmax {Dmax}"
    _same(_device(dec, syn), want, f"{what}, batch {B}")
    print(f"{what}: batch {B}, tile_syndromes {dec.info().tile_syndromes}, last_grid {dec.info().last_grid}")
    assert what_ran(dec) == (tier, S, tiles_of(B, S)) and tiles_of(B, S) >= 3
    Bp = ragged_prefix_of(S)
    assert Bp <= B and tiles_of(Bp, S) == 3 and (S == 1 or Bp % S != 0)
    _same(_device(dec, syn[:Bp]), _rows(want, slice(0, Bp)), f"{what}, batch {Bp}")
    assert dec.info().last_grid == 3
    if n in (96, 6144, 6432):
        _same(_host(dec, syn), want, f"{what}, host entry")
        assert dec.info().last_grid == tiles_of(B, S)
    dec.close()
    # ... and the same graph with half of the bits mirrored: pins of both signs
    mirrored, msyn, T1, Dmax, mwant = mirrored_case(n, S)
    dec = decoder(ldpc, H, mirrored, T1, Dmax)
    assert what_ran(dec) == (tier, S, 0)
    _same(_device(dec, msyn), mwant, f"{what}, mirrored, rounds of {T1}")
    assert what_ran(dec) == (tier, S, tiles_of(B, S))
    dec.close()


def test_the_unlimited_tier_forced_at_n_768(ldpc, gpu):
    """kernel_variant = 2 at a size between BB-72 and "too large for LDS": 165 syndromes, two tiles of 64 and one of 37."""
    H, prior, syn, T, Dmax, want = width_case(768, 64)
    dec = decoder(ldpc, H, prior, T, Dmax, variant=2)
    assert what_ran(dec) == (2, 64, 0) and syn.shape[0] == 165
    _same(_device(dec, syn), want, "n 768 forced tier 2")
    assert dec.info().last_grid == 3
    dec.close()


# ---- 2. ties across the threads of a lane ------------------------------------------------------------------------------------
TIE_WIDTHS = {192: 32, 384: 16, 768: 8}


def tie_preconditions(H, prior, syn, T, Dmax, what):
    """-> the rule's output.  Ties occur, and the rule restated with the highest index on a tie gives other LLR bit patterns in
    at least one column: a kernel that breaks a tie the other way shows."""
    low, high = DecimModel(H, prior, T, Dmax), DecimModel(H, prior, T, Dmax, tie="highest")
    want, other = frozen(low.decode(syn)), high.decode(syn)
    columns = int((want[4].view(np.int32) != other[4].view(np.int32)).any(axis=1).sum())
    print(f"{what}: {low.last_ties} of {int(want[3].sum())} decimations are ties; the other rule changes {columns} of {len(syn)} columns")
    assert low.last_ties > 0 and columns > 0, (what, low.last_ties, columns)
    assert 0 < want[1].sum() < len(syn) and ((want[1] == 1) & (want[3] > 0)).any()
    return want


@functools.lru_cache(maxsize=None)
def tie_case(n):
    """(3,6)-regular, the UNIFORM prior of 0.06, errors at 0.06 (seed 5), rounds of 3 and at most 4 decimations."""
    ldpc = _ldpc()
    S = TIE_WIDTHS[n]
    assert DECIM_TABLE[n][:2] == (1, S)
    H = ldpc.codes.parity_check_csc(n, 6, 3)
    prior = llr_of_probs(np.full(n, 0.06))
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(n, batch_of(S), 0.06, seed=5))
    return H, prior, syn, tie_preconditions(H, prior, syn, 3, 4, f"ties n {n}")


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", sorted(TIE_WIDTHS))
def test_the_lowest_index_wins_a_tie_between_threads_of_a_lane(ldpc, gpu, n, variant):
    """With a uniform prior the first sweeps leave many bits at the same |L|; at S = 32, 16 and 8 the tied bits of a lane are
    scanned by 16, 32 and 64 threads (16 in the unlimited tier), whose keys meet in the atomicMax."""
    S = TIE_WIDTHS[n] if variant == 1 else 64
    H, prior, syn, want = tie_case(n)
    dec = decoder(ldpc, H, prior, 3, 4, variant=variant)
    assert what_ran(dec) == (variant, S, 0)
    _same(_device(dec, syn), want, f"ties n {n} tier {variant} S {S}")
    assert dec.info().last_grid == tiles_of(syn.shape[0], S)
    dec.close()


@functools.lru_cache(maxsize=None)
def bb72_short_case():
    """BB-72 H_X, uniform prior 0.06, the 400 syndromes of errors at 0.06 of seed 3 (tests/test_gpu_decim.py), rounds of 3 and
    at most 6 decimations."""
    ldpc = _ldpc()
    Hx, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    H = sp.csc_matrix(np.asarray(Hx, dtype=np.uint8))
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 400, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    want = tie_preconditions(H, prior, syn, 3, 6, "ties BB-72")
    reuse_preconditions(want[1], None, 400, 64, (1,))
    return H, prior, syn, want


def test_bb72_ties_in_the_unlimited_tier(ldpc, gpu):
    """kernel_variant = 2: 16 threads share a lane.  All 400 syndromes, seven tiles."""
    H, prior, syn, want = bb72_short_case()
    dec = decoder(ldpc, H, prior, 3, 6, variant=2)
    assert what_ran(dec) == (2, 64, 0)
    _same(_device(dec, syn), want, "ties BB-72 tier 2")
    assert dec.info().last_grid == 7
    dec.close()


# ---- 3. D at whole words -------------------------------------------------------------------------------------------------------
WORD_GRAPHS = {32: (8, 4), 33: (11, 3), 64: (8, 4)}      # n -> (row weight, column weight) of the Gallager graph


@functools.lru_cache(maxsize=None)
def word_case(n):
    """A small Gallager graph, per-bit priors, rounds of ONE iteration and every bit free; 70 syndromes, 30 of sampled errors and
    40 arbitrary.  The rows of a Gallager block add up to the all-ones row, so an arbitrary syndrome whose blocks disagree in
    parity is matched by no error: such a lane pins bit after bit until all n are in D."""
    ldpc = _ldpc()
    wr, wc = WORD_GRAPHS[n]
    H = ldpc.codes.parity_check_csc(n, wr, wc)
    s = H.shape[0]
    rng = np.random.default_rng(100 + n)
    prior = llr_of_probs(rng.uniform(0.01, 0.3, n))
    assert len(set(prior.tolist())) == n
    syn = ldpc.codes.syndromes_of(H, (rng.random((70, n)) < 0.05).astype(np.uint8))
    syn[30:] = rng.integers(0, 2, size=(40, s))
    model = DecimModel(H, prior, 1, n)
    err, conv, its, ndec, L = want = frozen(model.decode(syn))
    D = model.last_D
    assert (ndec == n).any() and (conv[ndec == n] == 0).all() and int(its.max()) == n + 1, (n, int(ndec.max()))
    assert 0 < conv.sum() < 70 and ((conv == 1) & (ndec > 0)).any()
    for j in (31, 32, 63):      # the last bit of a word, the first of the next
        assert j >= n or D[:, j].any(), (n, j)
    assert np.array_equal(D.sum(axis=1), ndec) and D[ndec == n].all()
    return H, prior, syn, want


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", sorted(WORD_GRAPHS))
def test_every_bit_pinned_where_d_ends_on_a_word(ldpc, gpu, n, variant):
    """dw = ceil(n / 32) words of D a lane: 1 at n = 32, 2 at n = 33 (the second holds one bit) and at n = 64; batch 70 is a full
    tile of 64 and a ragged one."""
    H, prior, syn, want = word_case(n)
    dec = decoder(ldpc, H, prior, 1, n, variant=variant)
    assert what_ran(dec) == (variant, 64, 0)
    _same(_device(dec, syn), want, f"n {n} tier {variant}, device entry")
    assert dec.info().last_grid == 2
    _same(_host(dec, syn), want, f"n {n} tier {variant}, host entry")
    dec.close()


# ---- 4. a tile after another in one slot -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def c240_case():
    """The inputs of test_per_bit_priors_on_240_8_4 (tests/test_gpu_decim.py): rounds of 4, at most 12 decimations, batch 130 =
    nine tiles of 16 on chip, three of 64 in the unlimited tier.  The model's flags satisfy reuse_preconditions in the
    order of the columns as it is."""
    ldpc = _ldpc()
    H, probs, syn = _c240(ldpc)
    want = frozen(DecimModel(H, llr_of_probs(probs), 4, 12).decode(syn))
    reuse_preconditions(want[1], None, 130, 16, (1, 3))
    reuse_preconditions(want[1], None, 130, 64, (1,))
    assert ((want[1] == 1) & (want[3] > 0)).any() and ((want[1] == 0) & (want[3] == 12)).any()
    return H, probs, syn, want


@pytest.mark.parametrize("variant,cap", [(1, 1), (1, 3), (2, 1)], ids=["tier1-grid1", "tier1-grid3", "tier2-grid1"])
def test_240_8_4_nine_tiles_of_16_under_a_capped_grid(ldpc, gpu, monkeypatch, variant, cap):
    """A tile that follows another in the same LDS block or workspace slot must find D cleared through `rec_words + dw` rows of
    width S = 16.  The knob is read when the decoder is created; setting it selects the experiments build."""
    H, probs, syn, want = c240_case()
    S = 16 if variant == 1 else 64
    monkeypatch.setenv("LDPC_MS_GRID_MAX", str(cap))
    dec = ldpc.DecimatedMinSumDecoder(H, None, 4, channel_probs=probs, max_decimations=12, kernel_variant=variant)
    assert dec._L is ldpc._capi.lib(True) and what_ran(dec) == (variant, S, 0)
    what = f"(240,8,4) tier {variant} grid {cap}"
    _same(_device(dec, syn), want, what)
    assert dec.info().last_grid == cap < tiles_of(130, S) == (9 if variant == 1 else 3)
    _same(_device(dec, syn[100:130]), _rows(want, slice(100, 130)), what + ", columns 100:130")
    assert dec.info().last_grid == min(cap, tiles_of(30, S))
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_more_tiles_than_resident_workgroups_in_the_product_build(ldpc, gpu, monkeypatch, variant):
    """64 (2 CUs + 1) + 37 syndromes: the 400 known ones repeated with a roll of 13 per repetition, so that equal syndromes
    sit in other lanes and tiles; the expected output is the model's 400 results indexed the same way.  The grid must
    come out smaller than the tile count -- if the occupancy of the kernels ever makes that false, this fails."""
    import torch

    monkeypatch.delenv("LDPC_MS_GRID_MAX", raising=False)
    assert not ldpc._capi.knobs_in_env()
    H, prior, syn, want = bb72_short_case()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 * (2 * cus + 1) + 37
    b = np.arange(B)
    idx = (b + 13 * (b // 400)) % 400
    assert idx[400] == 13 and (idx[:400] == np.arange(400)).all()
    dec = decoder(ldpc, H, prior, 3, 6, variant=variant)
    assert dec._L is ldpc._capi.lib(False) and what_ran(dec) == (variant, 64, 0)
    got = _device(dec, syn[idx])
    info = dec.info()
    print(f"decimation tier {variant}: {cus} CUs, batch {B}, tiles {tiles_of(B, 64)}, last_grid {info.last_grid}")
    assert 0 < info.last_grid < tiles_of(B, 64), (info, B)
    _same(got, _rows(want, idx), f"tier {variant}, batch {B}")
    dec.close()


def test_handles_of_width_64_and_1_alive_together(ldpc, gpu):
    """The dynamic-LDS limit is raised per kernel, not per handle: the S = 64 handle (n = 96) and the S = 1 handle (n = 6144)
    decode alternately, then the wide one is closed and the narrow one decodes once more."""
    wide, narrow = width_case(96, 64), width_case(6144, 1)
    dec_w = decoder(ldpc, wide[0], wide[1], wide[3], wide[4])
    dec_n = decoder(ldpc, narrow[0], narrow[1], narrow[3], narrow[4])
    assert what_ran(dec_w) == (1, 64, 0) and what_ran(dec_n) == (1, 1, 0)
    Bw, Bn = wide[2].shape[0], narrow[2].shape[0]
    for turn in range(2):
        _same(_device(dec_w, wide[2]), wide[5], f"S 64, turn {turn}")
        assert dec_w.info().last_grid == tiles_of(Bw, 64)
        _same(_device(dec_n, narrow[2]), narrow[5], f"S 1, turn {turn}")
        assert dec_n.info().last_grid == Bn
    dec_w.close()
    _same(_device(dec_n, narrow[2]), narrow[5], "S 1 after the S 64 handle was closed")
    dec_n.close()


# ---- 5. the largest state the planner admits, for the whole family ------------------------------------------------------
# A (3,6)-regular core padded with isolated bits and empty checks until ONE syndrome takes exactly 159 KiB = 162816 bytes of
# dynamic LDS: with the static LDS of the kernels (at most 896 bytes) that is 128 bytes short of a CU's 160 KiB.
LANE_BYTES = {      # (s, n, rec_words) -> the bytes of one syndrome's state (tile_plan.hpp)
    "minsum": lambda s, n, rec: 4 * (n + rec) + s,
    "relay": lambda s, n, rec: 4 * (2 * n + rec + (n + 31) // 32) + s,
    "pauli": lambda s, n, rec: 4 * (2 * n + rec) + s,
    "decim": lambda s, n, rec: 4 * (n + rec + (n + 31) // 32) + s,
}
LARGEST_ITERS = 3
LARGEST_LEGS = [2, 1, 1]


def padding_of(kind, s, n, rec, empty):
    """The isolated bits that, with `empty` empty checks, bring the state of one syndrome of the core (s, n, rec_words) to
    exactly 159 KiB by the kernel's per-lane formula."""
    size = LANE_BYTES[kind]
    isolated = 0
    while size(s + empty, n + isolated + 1, rec) <= KIB159:
        isolated += 1
    assert size(s + empty, n + isolated, rec) == KIB159 == 162816, (kind, empty, isolated, size(s + empty, n + isolated, rec))
    return isolated


def padded(H, isolated, empty):
    """H with `empty` empty checks behind its rows and `isolated` bits of degree 0 behind its columns."""
    H = sp.csc_matrix(H)
    s, n = H.shape
    out = sp.csc_matrix((H.data, H.indices, np.concatenate([H.indptr, np.full(isolated, H.indptr[-1], dtype=H.indptr.dtype)])),
                        shape=(s + empty, n + isolated))
    assert out.nnz == H.nnz and np.diff(out.indptr)[n:].sum() == 0
    return out


def padded_inputs(H, isolated, empty, rate, seed):
    """-> (per-bit probabilities [n + isolated], syndromes [5][s + empty]).  The core's bits have probabilities around `rate`
    and the isolated ones of 0.35 ... 0.65 (priors of both signs and of small magnitude, so that err is not all 0 there
    and no decimation goes to a bit without a check); rows 0 ... 4 are sampled at 0.1, 0.1, 0.3, 1 and 1.9 times the core's
    probabilities.  Every empty check's entry is 0, but for the first empty check in row 0: that row can never converge."""
    s, n = H.shape
    rng = np.random.default_rng(seed)
    probs = np.concatenate([rate * rng.uniform(0.5, 1.5, n), rng.uniform(0.35, 0.65, isolated)])
    scale = np.array([0.1, 0.1, 0.3, 1.0, 1.9])
    e = (rng.random((5, n)) < probs[None, :n] * scale[:, None]).astype(np.uint8)
    syn = np.zeros((5, s + empty), dtype=np.uint8)
    syn[:, :s] = _ldpc().codes.syndromes_of(H, e)
    syn[0, s] = 1
    return probs, syn


def plans_at_the_edge(plan_of, s, n, rec):
    """(tier 1, S = 1, 162816 bytes) as it is; one more empty check: the unlimited tier by size, refused under variant 1."""
    assert plan_of(s, n, rec, 0) == (OK, 1, 1, KIB159) and plan_of(s, n, rec, 1) == (OK, 1, 1, KIB159)
    assert plan_of(s + 1, n, rec, 0)[:3] == (OK, 2, 64) and plan_of(s + 1, n, rec, 1)[0] == UNSUPPORTED


def both_outcomes(conv, what):
    assert conv[0] == 0 and 0 < conv.sum() < 5, (what, conv.tolist())


def decim_plan(s, n, rec, variant):
    got = lib_plan(s, n, rec, variant)
    return (OK, *got) if isinstance(got, tuple) else (got, -1, -1, -1)


@functools.lru_cache(maxsize=None)
def largest_case(kind):
    """min-sum, relay, decim -> (H, prior, syn, gammas | None, model output)."""
    ldpc = _ldpc()
    n0 = 6144 if kind == "relay" else 12288
    core = ldpc.codes.parity_check_csc(n0, 6, 3)
    empty = {"minsum": 16, "relay": 8, "decim": 24}[kind]
    isolated = padding_of(kind, n0 // 2, n0, 2 * n0, empty)
    if kind == "minsum":
        assert (isolated, 4 * (14588 + 24576) + 6160) == (2300, KIB159)
    if kind == "decim":
        assert (isolated, 4 * (14144 + 24576 + 442) + 6168) == (1856, KIB159)
    H = padded(core, isolated, empty)
    probs, syn = padded_inputs(core, isolated, empty, 0.05 if kind != "relay" else 0.02, n0 + len(kind))
    prior = llr_of_probs(probs)
    assert (prior[n0:] < 0).any() and (prior[n0:] > 0).any() and np.abs(prior[n0:]).max() < 1.0 < np.abs(prior[:n0]).min()
    g = None
    if kind == "minsum":
        want = MinSumModel(H, prior, LARGEST_ITERS).decode(syn)
    elif kind == "relay":
        g = gammas_of(len(LARGEST_LEGS), H.shape[1], 3)
        want = RelayModel(H, prior, g, LARGEST_LEGS, stop_after=1).decode(syn)
    else:
        want = DecimModel(H, prior, 2, 1).decode(syn)
        assert ((want[1] == 0) & (want[3] == 1)).any()
    frozen(want)
    both_outcomes(want[1], kind)
    assert want[0][:, n0:].any() and not want[0][:, n0:].all()      # the isolated bits: err = (prior <= 0), not all 0
    return H, prior, syn, g, want


@pytest.mark.parametrize("relay", [False, True], ids=["minsum", "relay"])
def test_the_largest_on_chip_state_launches_minsum_and_relay(ldpc, gpu, relay):
    kind = "relay" if relay else "minsum"
    H, prior, syn, g, want = largest_case(kind)
    s, n = H.shape
    rec = 4 * (3072 if relay else 6144)
    plans_at_the_edge(lambda s_, n_, r_, v: debug_plan("ldpc_debug_tile_plan", s_, n_, r_, int(relay), v), s, n, rec)
    legs = LARGEST_LEGS if relay else [LARGEST_ITERS]
    dec = make_decoder(ldpc, relay, H, prior, g, legs, stop_after=1)
    assert what_ran(dec) == (1, 1, 0)
    family_same(family_device(dec, relay, syn), rows_of(want, relay, slice(0, 5)), f"{kind} at 159 KiB a syndrome")
    assert what_ran(dec) == (1, 1, 5)
    dec.close()


def test_the_largest_on_chip_state_launches_decimation(ldpc, gpu):
    H, prior, syn, _, want = largest_case("decim")
    s, n = H.shape
    assert (s, n) == (6168, 14144)
    plans_at_the_edge(decim_plan, s, n, 4 * 6144)
    dec = decoder(ldpc, H, prior, 2, 1)
    assert what_ran(dec) == (1, 1, 0)
    _same(_device(dec, syn), want, "decimation at 159 KiB a syndrome")
    assert what_ran(dec) == (1, 1, 5)
    dec.close()


@functools.lru_cache(maxsize=None)
def largest_pauli_case():
    """Hx and Hz (3,6)-regular over 6144 qubits from different seeds, four empty checks behind each, isolated qubits behind the
    columns; per-qubit (px, py, pz), on the isolated qubits large enough for priors of both signs.
    -> (Hx, Hz, probs, sx, sz, model output)."""
    ldpc = _ldpc()
    n0, empty = 6144, 8
    cx, cz = ldpc.codes.parity_check_csc(n0, 6, 3, seed=1), ldpc.codes.parity_check_csc(n0, 6, 3, seed=2)
    isolated = padding_of("pauli", n0, n0, 4 * n0, empty)
    Hx, Hz = padded(cx, isolated, empty // 2), padded(cz, isolated, empty // 2)
    n, r = n0 + isolated, n0 // 2
    rng = np.random.default_rng(n)
    probs = np.concatenate([0.02 * rng.uniform(0.5, 1.5, (n0, 3)), rng.uniform(0.15, 0.32, (isolated, 3))])
    scale = np.array([0.1, 0.1, 0.3, 1.0, 1.9])
    edges = np.cumsum(probs[None, :n0, :] * scale[:, None, None], axis=2)
    pauli = (rng.random((5, n0, 1)) >= edges).sum(axis=2)                      # 0 = X, 1 = Y, 2 = Z, 3 = I
    ex, ez = (pauli <= 1).astype(np.uint8), ((pauli == 1) | (pauli == 2)).astype(np.uint8)
    sx, sz = np.zeros((5, r + empty // 2), dtype=np.uint8), np.zeros((5, r + empty // 2), dtype=np.uint8)
    sx[:, :r], sz[:, :r] = ldpc.codes.syndromes_of(cx, ez), ldpc.codes.syndromes_of(cz, ex)
    sz[0, r] = 1                                                                # an empty Hz check's entry: row 0 never converges
    priors = pauli_priors(probs)
    assert (priors[:, n0:] < 0).any() and (priors[:, n0:] > 0).any()
    want = frozen(PauliMinSumModel(Hx, Hz, priors, LARGEST_ITERS).decode(sx, sz))
    both_outcomes(want[2], "pauli")
    assert (want[0][:, n0:] | want[1][:, n0:]).any()                            # isolated qubits that are no I
    return Hx, Hz, probs, sx, sz, want


def test_the_largest_on_chip_state_launches_pauli(ldpc, gpu):
    Hx, Hz, probs, sx, sz, want = largest_pauli_case()
    n, s = Hx.shape[1], Hx.shape[0] + Hz.shape[0]
    plans_at_the_edge(lambda s_, n_, r_, v: debug_plan("ldpc_debug_pauli_tile_plan", s_, n_, r_, v), s, n, 4 * 6144)
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, LARGEST_ITERS, pauli_probs=probs, check=False)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (1, 1, 0)
    pauli_same(pauli_device(dec, sx, sz), want, "pauli at 159 KiB a syndrome")
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (1, 1, 5)
    dec.close()
