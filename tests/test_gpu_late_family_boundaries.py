"""Pinned record forms of the three newest kernels of the min-sum family -- guided decimation (decim_kernels.hpp), the Pauli
relay (pauli_relay_kernels.hpp) -- and of relay min-sum at the two degrees it was not yet pinned at, against their numpy
models (tests/decim_model.py, pauli_relay_model.py, relay_model.py): equality in every element, the LLRs as bit patterns,
no tolerance.  The graphs, priors and precondition functions are those of tests/test_gpu_family_boundaries.py (checks of
degree 31, 32, 33, 63, 64 and 65, the minimum at the last position alone, the top bit of a sign word set in some columns
and not in others); the entries and comparisons are those of the kernels' own suites.  Every case asserts ON THE MODEL or on
the priors alone, before the GPU is touched, that its input gets to the path it is there for
(tests/test_late_family_boundaries_cpu.py runs the same assertions without a GPU), decodes batch 65 -- one full tile and a
ragged one at every S <= 64 -- on both tiers, and asserts the tier, the width and the grid that ran.

  a  decimation, every bit free to be pinned (rounds of one iteration, clip 4): each wide check ends, in some lane, with its
     whole support in D -- the path `a == kMsNone` with `m1 == m2 == clip` --, its last bit pinned with either sign and its
     position 31 pinned
  b  the same graph with a loose clip and rounds of two iterations
  c  decimation with `clip` below every |prior| of the wide checks: only the signs and the pins are left
  d  Pauli relay on the record forms of BOTH sides (the `zrow` side had never written a five-word or per-edge record), four
     legs, one of them with negative gammas: `fresh ? 0 : rec[...]` at the start of three later legs
  e  the same with every value clamped
  f  relay min-sum at degrees 33 (mask `(1u << 1) - 1u`) and 64 (the whole high sign word) next to 31, 32, 63 and 65"""
import functools

import numpy as np
import pytest

import test_gpu_decim as t_decim
import test_gpu_pauli_relay as t_prelay
import test_gpu_relay as t_relay
from decim_model import DecimModel
from pauli_model import pauli_priors
from pauli_relay_model import PauliRelayModel
from relay_model import RelayModel
from test_gpu_family_boundaries import (B, F, HX_WIDE, HZ_WIDE, PAULI_N, WIDE, family_edges, family_preconditions, pauli_edges,
                                        pauli_edges_reach_their_paths, pauli_first_sweep)
from test_gpu_pauli import frozen

pytestmark = pytest.mark.gpu
N = 300


def ran_as_asked(kernel, S, grid, variant, what):
    """What the handle reports after a decode of batch 65: the tier asked for, a tile of at most 64 syndromes, and one
    workgroup per tile -- at least a full tile and a ragged one."""
    assert kernel == variant, f"{what}: tier {kernel}, asked for {variant}"
    assert 1 <= S <= 64 and grid == -(-B // S) >= 2, f"{what}: S {S}, grid {grid}"


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.int32)


# ---- a, b, c: decimation -----------------------------------------------------------------------------------------------------

def wide_check_clip():
    """Half the smallest nonzero |prior| among the bits of the six wide checks."""
    prior = family_edges()[2]
    mag = np.abs(np.concatenate([prior[first:first + deg] for first, deg in WIDE.values()]))
    return float(F(0.5) * mag[mag > 0].min())


# case -> (round_iters, max_decimations, alpha, clip)
def decim_settings(case):
    return {"a": (1, N, 0.75, 4.0), "b": (2, N, 1.0, 1e6), "c": (1, 40, 0.75, wide_check_clip())}[case]


@functools.lru_cache(maxsize=None)
def decim_want(case):
    """-> (the model's (err, conv, iters, decimated, L), its D [B][n])."""
    H, _, prior, syn = family_edges()[:4]
    T, Dmax, alpha, clip = decim_settings(case)
    model = DecimModel(H, prior, T, Dmax, alpha=alpha, clip=clip)
    want = model.decode(syn)
    D = model.last_D
    frozen(*want, D)
    return want, D


def decim_preconditions(case):
    """Every precondition of a decimation case, on the priors and on the model's outputs and D alone."""
    _, _, prior, syn = family_edges()[:4]
    T, Dmax, alpha, clip = decim_settings(case)
    (err, conv, its, ndec, L), D = decim_want(case)
    pin = F(2.0) * F(clip)
    assert np.array_equal(D.sum(axis=1), ndec) and (np.abs(L[D]) == pin).all()       # a bit of D reads +-2 clip, every one
    if case == "c":
        # on the priors alone: every first-sweep b of the six wide checks is +-clip (every message is +0, b is the clamped
        # prior), so `mag < m1` is never true, `a` stays kMsNone and the records hold alpha * clip twice
        assert 0 < clip < 0.1
        for i, (first, deg) in WIDE.items():
            b = np.minimum(np.maximum(prior[first:first + deg], -F(clip)), F(clip))
            assert (np.abs(b) == F(clip)).all(), f"check {i}: an edge is not clamped"
            assert (b < 0).sum() == (2 if deg > 32 else 1) and b[-1] < 0          # the signs are what is left: those of case a
        La = decim_want("a")[0][4]
        assert (bits(L) != bits(La)).any(axis=1).all(), "the clamp leaves a column as it was"
        assert D.any() and (ndec == Dmax).any()
        return
    family_preconditions(prior, syn, "base prior")                                # 1
    # b_k of sweep 1 is the clamped prior (at clip 4 a few large priors are cut; the small and the negative ones are not)
    family_preconditions(np.minimum(np.maximum(prior, -F(clip)), F(clip)), syn, "clamped prior")
    free = (conv == 1) & (ndec > 0) & (ndec < N)
    full = ndec == N
    assert free.any(), "no lane converges after a decimation"                      # 2
    assert (full & (conv == 0)).any(), "no lane ends with every bit pinned"        # 3: the |D| == n exit
    assert (int(conv.sum()), int(full.sum())) == ((31, 34) if case == "a" else (45, 20))
    if case == "b":
        return
    assert not ((conv == 1) & ~free).any()                                         # every converged lane was rescued by pins
    for i, (first, deg) in WIDE.items():                                           # 4
        whole = D[:, first:first + deg].all(axis=1)
        assert 43 <= whole.sum() <= 53, f"check {i}: fully pinned in {int(whole.sum())} lanes"
        last = first + deg - 1
        assert (D[:, last] & (L[:, last] < 0)).any() and (D[:, last] & (L[:, last] > 0)).any(), f"check {i}: the last bit is pinned with one sign only"
        if deg >= 32:
            assert (D[:, first + 31] & (L[:, first + 31] < 0)).any(), f"check {i}: position 31 is never pinned negative"


def decim_decoder(ldpc, case, variant):
    H, _, prior, _ = family_edges()[:4]
    T, Dmax, alpha, clip = decim_settings(case)
    return t_decim._decoder(ldpc, H, prior, T, Dmax, alpha=alpha, clip=clip, kernel_variant=variant)


def decim_case(ldpc, case, variant, host):
    syn = np.array(family_edges()[3])
    decim_preconditions(case)
    want = decim_want(case)[0]
    dec = decim_decoder(ldpc, case, variant)
    what = f"decimation case {case}, tier {variant}"
    t_decim._same(t_decim._device(dec, syn), want, what + ", device entry")
    info = dec.info()
    ran_as_asked(dec.kernel, info.tile_syndromes, info.last_grid, variant, what)
    if host:
        t_decim._same(t_decim._host(dec, syn), want, what + ", host entry")
        ran_as_asked(dec.kernel, dec.info().tile_syndromes, dec.info().last_grid, variant, what + ", host entry")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_decimation_on_the_record_forms_with_every_bit_free(ldpc, gpu, variant):
    """decim_kernels.hpp, its own copy of the record code: the masks at `d0 == 32` and `deg == 64`, the high sign word, the
    per-edge form with its second pass.  Rounds of one iteration and 300 decimations: 34 lanes run until |D| == n, so each
    wide check runs with all its bits pinned (every |b| clamped to clip 4: `a == kMsNone`, `m1 == m2 == clip`), and the pins
    land on the last position and on position 31."""
    decim_case(ldpc, "a", variant, host=True)


@pytest.mark.parametrize("variant", [1, 2])
def test_decimation_on_the_record_forms_with_loose_clip_and_longer_rounds(ldpc, gpu, variant):
    """clip 1e6 (a pin reads +-2e6 and is never clamped away), rounds of two iterations, alpha 1."""
    decim_case(ldpc, "b", variant, host=False)


@pytest.mark.parametrize("variant", [1, 2])
def test_decimation_on_the_record_forms_with_every_value_clamped(ldpc, gpu, variant):
    """clip = half the smallest |prior| of the wide checks: every first-sweep |b| is clip, `a` stays kMsNone, the records
    hold alpha * clip twice; only the signs and the pins (+-2 clip) remain."""
    decim_case(ldpc, "c", variant, host=True)


# ---- d, e: Pauli relay -------------------------------------------------------------------------------------------------------
PR_LEGS, PR_STOP = [6, 4, 4, 4], 3
PR_GAMMA_SEED = 5


@functools.lru_cache(maxsize=None)
def pauli_relay_gammas():
    """gammas_of(4, 300, seed=5) with leg 2 made negative: leg 0 at 0.125, legs 1 and 3 in (-0.24, 0.66), leg 2 in (-0.66, 0]."""
    g = t_prelay.gammas_of(4, PAULI_N, seed=PR_GAMMA_SEED)
    g[2] = -np.abs(g[2])
    assert (g[0] == F(0.125)).all() and (g[2] <= 0).all() and (g[2] < 0).sum() >= PAULI_N - 1 and (g[1] > 0).any() and (np.abs(g) < 1).all()
    frozen(g)
    return g


def pauli_clamp_clip():
    """Half the smallest |prior| of the three tables."""
    priors = pauli_priors(pauli_edges()[2])
    clip = float(F(0.5) * np.abs(priors).min())
    assert 0 < clip < np.abs(priors).min()
    return clip


@functools.lru_cache(maxsize=None)
def pauli_relay_want(alpha, clamped):
    Hx, Hz, probs, sx, sz = pauli_edges()
    clip = pauli_clamp_clip() if clamped else 1e6
    want = PauliRelayModel(Hx, Hz, pauli_priors(probs), pauli_relay_gammas(), PR_LEGS, alpha=alpha, clip=clip, stop_after=PR_STOP).decode(sx, sz)
    frozen(*want)
    return want


def pauli_relay_start_beliefs():
    """The G planes of the first check sweep of leg 0, by the header's rule, from the model's g0 and gammas: M is the prior,
    TX = TZ = +0.  They must equal the prior tables bitwise for the first-sweep preconditions of the fixture to apply."""
    Hx, Hz, probs, _, _ = pauli_edges()
    priors = pauli_priors(probs)
    model = PauliRelayModel(Hx, Hz, priors, pauli_relay_gammas(), PR_LEGS, stop_after=PR_STOP)
    zero = np.zeros(PAULI_N, dtype=F)
    LX, LY, LZ = (model.g0[k][0] + model.gammas[0] * priors[k] for k in range(3))
    G = (LX + zero, (LY + zero) + zero, LZ + zero)
    assert all(g.dtype == F for g in G)
    for name, g, p in zip("XYZ", G, priors):
        assert np.array_equal(bits(g), bits(p)), f"G{name} of leg 0 is not prior_{name.lower()} in {int((bits(g) != bits(p)).sum())} qubits"
    return priors


def pauli_relay_preconditions(alpha, clamped):
    Hx, Hz, probs, sx, sz = pauli_edges()
    priors = pauli_relay_start_beliefs()                                        # 1, 2
    want = pauli_relay_want(alpha, clamped)
    gx, gz, conv, its, sol, M = want
    if clamped:
        clip = pauli_clamp_clip()
        for Hd, zrow in ((Hx, False), (Hz, True)):                              # every first-sweep |b| of both sides is clip
            assert all((np.abs(b) == F(clip)).all() for b in pauli_first_sweep(priors, Hd, zrow, clip))
        loose = pauli_relay_want(alpha, False)
        assert (bits(M) != bits(loose[5])).any(axis=(1, 2)).all(), "the clamp leaves a column as it was"
        assert not conv.any() and (its == sum(PR_LEGS)).all() and not sol.any()   # every lane runs all four legs to the end
        return
    pauli_edges_reach_their_paths()                                             # (clip 1e6: b is not clamped)
    for wide, Hd in ((HX_WIDE, Hx), (HZ_WIDE, Hz)):
        assert sorted(int(Hd[i].sum()) for i in wide) == [31, 32, 33, 63, 64, 65]
    assert 0 < conv.sum() < B, int(conv.sum())                                  # 3
    assert set(sol.tolist()) == {0, 1, 2, 3}, np.bincount(sol).tolist()
    assert len(set(its.tolist())) >= 4, sorted(set(its.tolist()))
    assert t_prelay.best_is_not_the_final_decision(want) >= 1
    if alpha == 0.75:
        assert (int(conv.sum()), np.bincount(sol).tolist(), len(set(its.tolist())), t_prelay.best_is_not_the_final_decision(want)) == \
            (10, [55, 8, 1, 1], 5, 3)


def pauli_relay_case(ldpc, alpha, clamped, variant):
    Hx, Hz, probs, sx, sz = pauli_edges()
    pauli_relay_preconditions(alpha, clamped)
    want = pauli_relay_want(alpha, clamped)
    clip = pauli_clamp_clip() if clamped else 1e6
    # the sides of the fixture do not commute: check=False
    dec = ldpc.PauliRelayMinSumDecoder(Hx, Hz, None, PR_LEGS[0], pauli_probs=probs, legs=len(PR_LEGS), leg_iters=PR_LEGS[1],
                                       gammas=pauli_relay_gammas(), stop_after=PR_STOP, alpha=alpha, clip=clip, kernel_variant=variant,
                                       check=False)
    assert dec.leg_iters.tolist() == PR_LEGS and np.array_equal(bits(dec.gammas), bits(pauli_relay_gammas()))
    assert all(np.array_equal(bits(got), bits(p)) for got, p in zip((dec.prior_x, dec.prior_y, dec.prior_z), pauli_priors(probs)))
    assert (dec.n, dec.rows_x, dec.rows_z) == (PAULI_N, 30, 30)
    what = f"Pauli relay alpha {alpha} clip {clip}, tier {variant}"
    t_prelay.same(t_prelay.device_entry(dec, sx, sz), want, what + ", device entry")
    ran_as_asked(dec.kernel, dec.tile_syndromes, dec.last_grid, variant, what)
    t_prelay.same(t_prelay.host_entry(dec, sx, sz), want, what + ", host entry")
    ran_as_asked(dec.kernel, dec.tile_syndromes, dec.last_grid, variant, what + ", host entry")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_pauli_relay_record_forms_at_degrees_31_to_65_on_both_sides(ldpc, gpu, alpha, variant):
    """pauli_relay_kernels.hpp, a third copy of the record code with `fresh ? 0 : rec[...]` on every read of the old record:
    the records of Hx rows and of Hz rows (`zrow`) in the four-word, five-word and per-edge form, through four legs -- the
    first sweep of each later leg reads the records a full-width leg left behind as if they were zero."""
    pauli_relay_case(ldpc, alpha, False, variant)


@pytest.mark.parametrize("variant", [1, 2])
def test_pauli_relay_record_forms_with_every_value_clamped(ldpc, gpu, variant):
    """clip below the smallest |prior|: no lane converges and all run 18 iterations; the case is about the signs and the
    `fresh` start of three later legs on full-width records."""
    pauli_relay_case(ldpc, 1.0, True, variant)


# ---- f: relay min-sum ---------------------------------------------------------------------------------------------------------
RL_LEGS = [8, 6, 6]


@functools.lru_cache(maxsize=None)
def relay_want():
    H, _, prior, syn = family_edges()[:4]
    g = t_relay._gammas(3, N, seed=8)
    want = RelayModel(H, prior, g, RL_LEGS, stop_after=2).decode(syn)
    frozen(g, *want)
    return g, want


def relay_preconditions():
    H, _, prior, syn = family_edges()[:4]
    g, want = relay_want()
    family_preconditions(prior, syn, "base prior")
    # the belief the first sweep of leg 0 reads, g0 + gamma * M with M the prior, keeps every property of the prior
    model = RelayModel(H, prior, g, RL_LEGS, stop_after=2)
    family_preconditions((model.g0[0] + model.gammas[0] * prior).astype(F), syn, "leg-0 start belief")
    err, conv, its, sol, M = want
    assert conv.any() and not conv.all(), "the model finds a solution for every column or for none"
    assert (its > RL_LEGS[0]).any(), "no column goes beyond the first leg"
    assert (int(conv.sum()), int((its > RL_LEGS[0]).sum()), np.bincount(sol).tolist()) == (18, 62, [47, 8, 10])


@pytest.mark.parametrize("variant", [1, 2])
def test_relay_record_forms_at_degrees_33_and_64(ldpc, gpu, variant):
    """relay_kernels.hpp at the two degrees tests/test_gpu_model_boundaries.py leaves out: 33 (one bit of the high sign word)
    and 64 (all of it), next to 31, 32, 63 and 65 on the same graph."""
    H, _, prior, syn = family_edges()[:4]
    relay_preconditions()
    g, want = relay_want()
    dec = t_relay._decoder(ldpc, H, prior, g, RL_LEGS, stop_after=2, kernel_variant=variant)
    what = f"relay, tier {variant}"
    t_relay._same(t_relay._device(dec, np.array(syn)), want, what + ", device entry")
    ran_as_asked(dec.kernel, dec.info().tile_syndromes, dec.info().last_grid, variant, what)
    t_relay._same(t_relay._host(dec, np.array(syn)), want, what + ", host entry")
    ran_as_asked(dec.kernel, dec.info().tile_syndromes, dec.info().last_grid, variant, what + ", host entry")
    dec.close()
