"""Pauli relay min-sum decoder on the GPU against the numpy model of its rule (tests/pauli_relay_model.py): equality in
every element through both entries -- gx, gz, flags, iteration counts, solution counts, and the three LLR planes as bit
patterns.  The arithmetic has no division and no transcendental function, so there is no tolerance.  What ran is read back
and asserted (`.kernel`, `.tile_syndromes`, `.last_grid`), so a case that misses its tier or width fails instead of passing
on another path, and every case asserts ON THE MODEL, before anything touches the GPU, that its batch holds what it is
there for (lanes that stop in different legs, several solutions, a best that is not the decision on the final M).  Every
model result is computed once, shared, and never written to.  The widths: tests/test_gpu_pauli_relay_widths.py."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
from pauli_model import PauliMinSumModel, depolarizing_priors, pauli_priors
from pauli_relay_model import PauliRelayModel
from test_gpu_pauli import bb72, bb72_syndromes, frozen, tiles_of

pytestmark = pytest.mark.gpu
F = np.float32


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


# ---- decoders, entries and comparison ---------------------------------------------------------------------------------------

def gammas_of(legs, n, seed=0):
    """Leg 0 at 0.125, legs 1... uniform in (-0.24, 0.66): what the constructor draws by default."""
    g = np.empty((legs, n), dtype=F)
    g[0] = F(0.125)
    g[1:] = np.random.default_rng(seed).uniform(-0.24, 0.66, (legs - 1, n)).astype(F)
    return g


def raw_decoder(ldpc, Hx, Hz, priors, gammas, leg_iters, stop_after=1, variant=0, alpha=0.75, clip=1e6):
    """A PauliRelayMinSumDecoder over ldpc_pauli_relay_create with ANY leg_iters (the constructor spells only
    [max_iters, leg_iters, leg_iters, ...]); priors [3][n] float32."""
    from ldpcdecoders_jl_amd._host import _pattern_of, css_pattern

    d = object.__new__(ldpc.PauliRelayMinSumDecoder)
    Mx, Mz = _pattern_of(Hx), _pattern_of(Hz)
    d.sparse_Hx, d.sparse_Hz = Mx, Mz
    d.n, d.rows_x, d.rows_z, d.device = int(Mx.shape[1]), int(Mx.shape[0]), int(Mz.shape[0]), 0
    d.prior_x, d.prior_y, d.prior_z = (np.ascontiguousarray(priors[k], dtype=F) for k in range(3))
    d.gammas = np.ascontiguousarray(gammas, dtype=F)
    d.leg_iters = np.ascontiguousarray(leg_iters, dtype=np.int32)
    assert d.gammas.shape == (len(d.leg_iters), d.n)
    pat_x, pat_z = css_pattern(Mx), css_pattern(Mz)
    o = ldpc._capi.PauliRelayOptions()
    o.device, o.alpha, o.clip, o.kernel_variant, o.stop_after = 0, alpha, clip, variant, stop_after
    L = ldpc._capi.lib_for(None)
    d._create(L, L.ldpc_pauli_relay_create, d.n, ctypes.byref(pat_x), ctypes.byref(pat_z), d.prior_x.ctypes.data, d.prior_y.ctypes.data,
              d.prior_z.ctypes.data, len(d.leg_iters), d.gammas.ctypes.data, d.leg_iters.ctypes.data, ctypes.byref(o))
    return d


def device_entry(dec, sx, sz, want_llr=True, want_iters=True, want_sol=True):
    """-> (gx, gz, conv, iters | None, solutions | None, llr | None), every output buffer pre-filled with a value no
    decode writes."""
    import torch

    B = sx.shape[0]
    d_sx = torch.from_numpy(np.array(sx, dtype=np.uint8, order="C")).cuda()      # (a copy: the shared inputs are read-only)
    d_sz = torch.from_numpy(np.array(sz, dtype=np.uint8, order="C")).cuda()
    gx = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    gz = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, 3, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    sol = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_sol else None
    dec.decode_batch_device(d_sx, d_sz, gx, gz, conv, llr, its, sol)
    torch.cuda.synchronize()
    return (gx.cpu().numpy(), gz.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy() if want_iters else None,
            sol.cpu().numpy() if want_sol else None, llr.cpu().numpy() if want_llr else None)


def host_entry(dec, sx, sz, want_llr=True, want_sol=True):
    out = dec.decode_batch_host(sx, sz, want_llr=want_llr, want_solutions=want_sol)
    assert len(out) == (6 if want_sol else 5) and (out[3] is None) == (not want_llr)
    gx, gz, conv, llr, its = out[:5]
    return gx, gz, conv, its, out[5] if want_sol else None, llr


def same(got, want, what, idx=slice(None)):
    """got = (gx, gz, conv, iters | None, solutions | None, llr f64 | None) of an entry, want = the model's
    (gx, gz, conv, iters, solutions, M f32)."""
    gx, gz, conv, its, sol, llr = got
    mgx, mgz, mconv, mits, msol, mM = (x[idx] for x in want)
    assert gx.shape == mgx.shape and np.array_equal(gx, mgx), f"{what}: gx differs in {int((gx != mgx).any(axis=1).sum())} of {len(gx)} columns"
    assert gz.shape == mgz.shape and np.array_equal(gz, mgz), f"{what}: gz differs in {int((gz != mgz).any(axis=1).sum())} of {len(gz)} columns"
    assert np.array_equal(conv, mconv), f"{what}: converged flags differ in columns {np.nonzero(conv != mconv)[0][:8].tolist()}"
    if its is not None:
        assert its.dtype == np.int32 and np.array_equal(its, mits), f"{what}: iteration counts differ in columns {np.nonzero(its != mits)[0][:8].tolist()}"
    if sol is not None:
        assert sol.dtype == np.int32 and np.array_equal(sol, msol), f"{what}: solution counts differ in columns {np.nonzero(sol != msol)[0][:8].tolist()}"
    if llr is not None:
        assert llr.dtype == np.float64 and llr.shape == mM.shape
        assert np.array_equal(llr.view(np.int64), mM.astype(np.float64).view(np.int64)), f"{what}: LLR bit patterns differ"


def best_is_not_the_final_decision(want):
    """The columns whose output is not the decision on the M they ended with."""
    gx, gz, _, _, _, M = want
    ex, ez = PauliMinSumModel._decide(M[:, 0], M[:, 1], M[:, 2])
    return int((((gx != 0) != ex).any(axis=1) | ((gz != 0) != ez).any(axis=1)).sum())


# ---- BB-72: the cases of the table ------------------------------------------------------------------------------------------
# name -> (leg_iters, stop_after, per-qubit rates?, clip, negative leg?)
CASES = {
    "three-solutions": ([6, 4, 4, 4], 3, False, 1e6, False),
    "skipped-leg": ([5, 0, 3, 3, 3], 2, False, 1e6, False),
    "never-reached": ([3, 2, 2], 5, False, 1e6, False),
    "per-qubit-rates": ([6, 4, 4, 4], 3, True, 1e6, False),
    "negative-leg": ([6, 4, 4, 4], 3, False, 1e6, True),
    "clip-8": ([6, 4, 4, 4], 3, False, 8.0, False),
}
# name -> (converged, the histogram of `solutions`, distinct iteration counts | None, max iterations | None, columns where
# best is not the decision on the final M): what the model gives on these inputs, asserted before any comparison
EXPECT = {
    "three-solutions": (196, [4, 5, 6, 185], 16, 18, 8),
    "skipped-leg": (194, [6, 7, 187], None, 14, 4),
    "never-reached": (181, [19, 8, 25, 148], None, 7, 5),
    "per-qubit-rates": (197, [3, 4, 6, 187], None, None, 7),
}


def case_inputs(name):
    """-> (priors [3][n], pauli_probs | None, gammas, leg_iters, stop_after, clip)."""
    legs, stop_after, rates, clip, negative = CASES[name]
    probs = np.random.default_rng(3).uniform(0.005, 0.04, (72, 3)) if rates else None
    priors = pauli_priors(probs) if rates else depolarizing_priors(72, 0.06)
    g = gammas_of(len(legs), 72)
    if negative:
        g[1] = -np.abs(g[1]) - F(0.05)          # leg 1 wholly negative, inside (-0.71, -0.05)
        assert (g[1] < 0).all() and (g[1] > -1).all()
    return priors, probs, g, legs, stop_after, clip


@functools.lru_cache(maxsize=None)
def bb72_case(name):
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    priors, _, g, legs, stop_after, clip = case_inputs(name)
    want = PauliRelayModel(Hx, Hz, priors, g, legs, clip=clip, stop_after=stop_after).decode(sx, sz)
    frozen(*want)
    return want


def make(ldpc, name, variant=0):
    """The decoder of a case: through the constructor where it can spell the legs, else over the C entry."""
    Hx, Hz = bb72()
    priors, probs, g, legs, stop_after, clip = case_inputs(name)
    if len(set(legs[1:])) > 1:
        return raw_decoder(ldpc, Hx, Hz, priors, g, legs, stop_after=stop_after, variant=variant, clip=clip)
    return ldpc.PauliRelayMinSumDecoder(Hx, Hz, None if probs is not None else 0.06, legs[0], pauli_probs=probs, legs=len(legs),
                                        leg_iters=legs[1], gammas=g, stop_after=stop_after, clip=clip, kernel_variant=variant)


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bb72_equals_the_model(ldpc, gpu, name, variant):
    """2976 B a syndrome: S = 16 on chip by size, 64 in the unlimited tier.  Device and host entries."""
    sx, sz = bb72_syndromes()
    want = bb72_case(name)
    gx, gz, conv, its, sol, M = want
    got = (int(conv.sum()), np.bincount(sol).tolist(), len(set(its.tolist())), int(its.max()), best_is_not_the_final_decision(want))
    print(f"{name}: converged {got[0]} of 200, solutions {got[1]}, {got[2]} iteration counts up to {got[3]}, best != final in {got[4]}")
    if name in EXPECT:
        e = EXPECT[name]
        assert got[:2] == e[:2] and got[4] == e[4] and e[2] in (None, got[2]) and e[3] in (None, got[3]), (name, got, e)
    else:
        assert 0 < got[0] < 200 and len(got[1]) == 4 and min(got[1]) > 0 and got[4] > 0, (name, got)
    if name == "clip-8":
        assert (M.view(np.int32) != bb72_case("three-solutions")[5].view(np.int32)).any(axis=(1, 2)).sum() >= 50   # the clamp is exercised
    if name == "per-qubit-rates":
        priors = case_inputs(name)[0]
        assert (priors[0] != priors[1]).all() and (priors[1] != priors[2]).all()      # the three weights of a qubit differ
    dec = make(ldpc, name, variant)
    tier, S = (1, 16) if variant == 0 else (2, 64)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, 0) and (dec.n, dec.rows_x, dec.rows_z) == (72, 36, 36)
    what = f"BB-72 {name} tier {tier}"
    same(device_entry(dec, sx, sz), want, what + ", device entry")
    assert dec.last_grid == tiles_of(200, S) and dec.info().device == 0 and dec.info().kernel == tier and dec.info().tile_syndromes == S
    same(host_entry(dec, sx, sz), want, what + ", host entry")
    dec.close()
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_defaults_converge_on_every_syndrome(ldpc, gpu, variant):
    """The constructor's defaults -- 9 legs of 30, 20, ... iterations, its own gammas -- on the same batch."""
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want = PauliRelayModel(Hx, Hz, depolarizing_priors(72, 0.06), gammas_of(9, 72), [30] + [20] * 8).decode(sx, sz)
    assert int(want[2].sum()) == 200 and (want[4] == 1).all() and int(want[3].max()) > 30      # some columns need a later leg
    dec = ldpc.PauliRelayMinSumDecoder(Hx, Hz, 0.06, kernel_variant=variant)
    assert np.array_equal(dec.gammas.view(np.int32), gammas_of(9, 72).view(np.int32)) and dec.leg_iters.tolist() == [30] + [20] * 8
    same(device_entry(dec, sx, sz), want, f"BB-72 defaults tier {variant}")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_the_eight_masks_of_optional_outputs_and_slices(ldpc, gpu, variant):
    """llr, iters and solutions present or NULL in every combination through the device entry, the four of the host entry;
    then slices of the batch on the same handle: the state a tile finds is what the call before left."""
    sx, sz = bb72_syndromes()
    want = bb72_case("three-solutions")
    dec = make(ldpc, "three-solutions", variant)
    S = dec.tile_syndromes
    for mask in range(8):
        llr, its, sol = bool(mask & 1), bool(mask & 2), bool(mask & 4)
        got = device_entry(dec, sx, sz, want_llr=llr, want_iters=its, want_sol=sol)
        assert (got[5] is not None, got[3] is not None, got[4] is not None) == (llr, its, sol)
        same(got, want, f"tier {variant}, device entry, mask {mask}")
    for llr in (False, True):
        for sol in (False, True):
            same(host_entry(dec, sx, sz, want_llr=llr, want_sol=sol), want, f"tier {variant}, host entry, llr {llr} solutions {sol}")
    for lo, hi in ((100, 200), (0, 200), (37, 70), (5, 6)):
        same(device_entry(dec, sx[lo:hi], sz[lo:hi]), want, f"tier {variant}, columns {lo}:{hi}", slice(lo, hi))
        assert dec.last_grid == tiles_of(hi - lo, S)
    same(host_entry(dec, sx[199:], sz[199:]), want, f"tier {variant}, one column through the host entry", slice(199, 200))
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_syndrome_entries_2_and_3(ldpc, gpu, variant):
    """An entry that is not 0 counts as 1."""
    sx, sz = bb72_syndromes()
    want = bb72_case("three-solutions")
    wx, wz = sx.copy(), sz.copy()
    wx[wx == 1] = np.where(np.arange((wx == 1).sum()) % 2 == 0, 2, 3)
    wz[wz == 1] = np.where(np.arange((wz == 1).sum()) % 3 == 0, 255, 128)
    assert set(np.unique(wx)) == {0, 2, 3} and set(np.unique(wz)) == {0, 128, 255}
    dec = make(ldpc, "three-solutions", variant)
    same(device_entry(dec, wx, wz), want, f"tier {variant}, entries 2, 3, 128, 255")
    same(host_entry(dec, wx, wz), want, f"tier {variant}, entries 2, 3, 128, 255, host entry")
    dec.close()


def test_every_leg_of_zero_iterations_and_batch_zero(ldpc, gpu):
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    priors = depolarizing_priors(72, 0.06)
    dec = raw_decoder(ldpc, Hx, Hz, priors, gammas_of(3, 72), [0, 0, 0], stop_after=2)
    want = PauliRelayModel(Hx, Hz, priors, gammas_of(3, 72), [0, 0, 0], stop_after=2).decode(sx, sz)
    assert all(not x.any() for x in want)
    for got in (device_entry(dec, sx, sz), host_entry(dec, sx, sz)):
        same(got, want, "every leg 0")
        assert not got[5].view(np.int64).any()                      # +0, not -0
    assert dec.last_grid == 0                                       # no kernel ran
    L = dec._L
    assert L.ldpc_pauli_relay_decode_batch(dec._h, 0, None, None, None, None, None, None, None, None) == 0     # batch 0: nothing touched
    assert L.ldpc_pauli_relay_decode_batch_device(dec._h, 0, None, None, None, None, None, None, None, None, None) == 0
    assert L.ldpc_pauli_relay_decode_batch(dec._h, -1, None, None, None, None, None, None, None, None) == 1
    assert L.ldpc_pauli_relay_decode_batch(dec._h, 1, None, None, None, None, None, None, None, None) == 1
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("max_iters", [1, 30])
def test_one_leg_at_gamma_zero_equals_the_pauli_min_sum_decoder_on_the_gpu(ldpc, gpu, max_iters, variant):
    """The consequence the header states, between the two kernels: every output bit, the LLR planes included."""
    from test_gpu_pauli import device_entry as pauli_device

    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    ref = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, max_iters, kernel_variant=variant)
    gx, gz, conv, its, llr = pauli_device(ref, sx, sz)
    ref.close()
    assert 0 < conv.sum() < 200
    dec = ldpc.PauliRelayMinSumDecoder(Hx, Hz, 0.06, max_iters, legs=1, gammas=np.zeros((1, 72), dtype=F), kernel_variant=variant)
    got = device_entry(dec, sx, sz)
    dec.close()
    assert np.array_equal(got[0], gx) and np.array_equal(got[1], gz) and np.array_equal(got[2], conv) and np.array_equal(got[3], its)
    assert np.array_equal(got[4], conv.astype(np.int32)) and np.array_equal(got[5].view(np.int64), llr.view(np.int64))
    want = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, 0.06), max_iters).decode(sx, sz)
    assert np.array_equal(got[5].view(np.int64), want[4].astype(np.float64).view(np.int64))


# ---- record forms, empty nodes -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def irregular_case():
    """n = 72.  Hx: the all-ones row over qubits 0 .. 69 (degree 70: one word per edge), the row over qubits 0 .. 39 (degree
    40: the 5-word record), an empty row.  Hz: the pairs (2 k, 2 k + 1) for k < 35 (4-word records; every pair lies inside or
    outside both rows, so the sides commute) and an empty row.  Qubits 70 and 71 are in no check; qubit 71 has negative
    priors.  215 record words; 4 (432 + 215 + 6) + 39 = 2651 B a syndrome: S = 16.  The first column sets the entry of the
    empty Hx row, the second that of the empty Hz row: neither can ever be matched."""
    n = 72
    Hx = np.zeros((3, n), dtype=np.uint8)
    Hx[0, :70], Hx[1, :40] = 1, 1
    Hz = np.zeros((36, n), dtype=np.uint8)
    Hz[np.arange(70) // 2, np.arange(70)] = 1
    ex, ez = cm.sample(n, 90, 0.04, seed=72)
    sx, sz = cm.syndromes(sp.csc_matrix(Hx), sp.csc_matrix(Hz), ex, ez)
    sx[0, 2], sz[1, 35] = 1, 3
    rng = np.random.default_rng(72)
    probs = rng.uniform(0.01, 0.08, (n, 3))                       # per-qubit priors: the minima of the wide rows are distinct
    probs[71] = [0.4, 0.3, 0.2]
    g = gammas_of(3, n, seed=4)
    want = PauliRelayModel(Hx, Hz, pauli_priors(probs), g, [4, 3, 3], stop_after=2).decode((sx != 0), (sz != 0))
    frozen(sx, sz, *want)
    return Hx, Hz, probs, g, sx, sz, want


@pytest.mark.parametrize("variant", [1, 2])
def test_irregular_graph_every_record_form_empty_checks_and_isolated_qubits(ldpc, gpu, variant):
    Hx, Hz, probs, g, sx, sz, want = irregular_case()
    gx, gz, conv, its, sol, M = want
    assert not conv[:2].any() and 0 < conv.sum() < 90 and len(set(sol.tolist())) == 3 and len(set(its.tolist())) >= 4
    assert (gx[:, 71] | gz[:, 71]).all() and not gx[:, 70].any() and not gz[:, 70].any()
    dec = ldpc.PauliRelayMinSumDecoder(Hx, Hz, None, 4, pauli_probs=probs, legs=3, leg_iters=3, gammas=g, stop_after=2, kernel_variant=variant)
    assert (dec.kernel, dec.tile_syndromes) == ((1, 16) if variant == 1 else (2, 64))
    same(device_entry(dec, sx, sz), want, f"irregular graph, tier {variant}")
    assert dec.last_grid == tiles_of(90, dec.tile_syndromes)
    same(host_entry(dec, sx, sz), want, f"irregular graph, tier {variant}, host entry")
    dec.close()


# ---- tile after tile in one slot ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_tile_after_tile_in_one_slot_under_a_capped_grid(ldpc, gpu, monkeypatch, variant, cap):
    """One handle of the experiments build, three calls in a row on `cap` workgroups: every state a tile finds -- G, M, the
    records, best, the per-lane registers -- is what the tile or the call before left there.  The knob is read when the
    decoder is created; setting it selects the experiments build."""
    sx, sz = bb72_syndromes()
    want = bb72_case("three-solutions")
    monkeypatch.setenv("LDPC_MS_GRID_MAX", str(cap))
    dec = make(ldpc, "three-solutions", variant)
    S = 16 if variant == 1 else 64
    assert dec._L is ldpc._capi.lib(True) and (dec.kernel, dec.tile_syndromes, dec.last_grid) == (variant, S, 0)
    for lo, hi in ((136, 200), (0, 200), (50, 150)):
        same(device_entry(dec, sx[lo:hi], sz[lo:hi]), want, f"tier {variant} grid {cap}, columns {lo}:{hi}", slice(lo, hi))
        assert dec.last_grid == min(cap, tiles_of(hi - lo, S))
    assert cap < tiles_of(200, S)
    dec.close()


# ---- the trials driver -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def trials_case():
    """600 trials of BB-72 at depolarizing 0.06, seed 9: css_trials_model sample -> PauliRelayModel -> model score."""
    ldpc = _ldpc()
    Hx, Hz = bb72()
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    ex, ez = cm.sample(72, 600, 0.06, seed=9)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    gx, gz, conv, its, sol, _ = PauliRelayModel(Hx, Hz, depolarizing_priors(72, 0.06), gammas_of(3, 72), [4, 3, 3]).decode(sx, sz)
    _, counts = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    nc = int((conv == 0).sum())
    return ldpc.CSSTrialResult(trials=int(counts[0]), block_errors=int(counts[1]), syndrome_mismatches=int(counts[2]),
                               logical_errors=int(counts[3]), logical_x_errors=int(counts[4]), logical_z_errors=int(counts[5]),
                               not_converged_hx=nc, not_converged_hz=nc)


def test_run_css_joint_trials_drives_the_decoder_unchanged(ldpc, gpu):
    Hx, Hz = bb72()
    want = trials_case()
    assert want.trials == 600 and 0 < want.logical_errors < 600 and 0 < want.not_converged_hx < 600
    dec = ldpc.PauliRelayMinSumDecoder(Hx, Hz, 0.06, 4, legs=3, leg_iters=3)
    a = ldpc.run_css_joint_trials(dec, 600, 0.06, batch=256, seed=9)
    b = ldpc.run_css_joint_trials(dec, 600, 0.06, batch=600, seed=9)
    assert a == b == want, (a, b, want)
    assert ldpc.run_css_joint_trials(dec, 0, 0.06).trials == 0
    dec.close()
