"""Relay min-sum decoder on the GPU against the numpy model of its rule (tests/relay_model.py): equality in every element
-- errors, flags, iteration counts, solution counts, and the LLRs as bit patterns -- on both tiers, through the device
entry and the host entry, on the smallest shapes that reach every code path: lanes of one tile in different legs, legs
that end by a solution and by exhaustion, tiles of 64 / 16 syndromes, ragged tiles, every record form, the clamps, and
the compositions with the trials loops and the OSD step."""
import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import trials_model as tm
from minsum_model import MinSumModel, llr_of_probs
from osd_model import osd_model_postprocess
from relay_model import RelayModel, weights_of

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5
NINE_LEGS = [30] + [20] * 8


def _bb72(ldpc):
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx, dtype=np.uint8)), sp.csc_matrix(np.asarray(Hz, dtype=np.uint8))


def _gammas(legs, n, seed=5):
    g = np.empty((legs, n), dtype=np.float32)
    g[0] = 0.125
    g[1:] = np.random.default_rng(seed).uniform(-0.24, 0.66, size=(legs - 1, n)).astype(np.float32)
    return g


def _decoder(ldpc, H, prior, gammas, leg_iters, **kw):
    """A RelayMinSumDecoder with the [legs][n] gammas and the per-leg iteration counts of a model."""
    assert len(set(leg_iters[1:])) <= 1
    return ldpc.RelayMinSumDecoder(H, None, int(leg_iters[0]), channel_llr=prior, legs=len(leg_iters),
                                   leg_iters=int(leg_iters[1]) if len(leg_iters) > 1 else 0, gammas=gammas, **kw)


def _device(dec, syn, want_llr=True, want_iters=True, want_sol=True):
    import torch

    B = syn.shape[0]
    d_syn = torch.from_numpy(np.ascontiguousarray(syn, dtype=np.uint8)).cuda()
    err = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    sol = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_sol else None
    dec.decode_batch_device(d_syn, err, conv, llr, its, sol)
    torch.cuda.synchronize()
    return (err.cpu().numpy(), conv.cpu().numpy(), llr.cpu().numpy() if want_llr else None,
            its.cpu().numpy() if want_iters else None, sol.cpu().numpy() if want_sol else None)


def _host(dec, syn):
    return dec.decode_batch_host(syn, want_llr=True, want_solutions=True)


def _same(got, want, what=""):
    """got = (err, conv, llr f64 | None, iters | None, solutions | None) of the library, want = (err, conv, iters,
    solutions, M f32) of the model."""
    err, conv, llr, its, sol = got
    merr, mconv, mits, msol, mM = want
    assert np.array_equal(err, merr), f"{what}: errors differ in {int((err != merr).any(axis=1).sum())} columns"
    assert np.array_equal(conv, mconv), f"{what}: converged flags differ"
    if its is not None:
        assert its.dtype == np.int32 and np.array_equal(its, mits), f"{what}: iteration counts differ"
    if sol is not None:
        assert sol.dtype == np.int32 and np.array_equal(sol, msol), f"{what}: solution counts differ"
    if llr is not None:
        assert llr.dtype == np.float64
        assert np.array_equal(llr.view(np.int64), mM.astype(np.float64).view(np.int64)), f"{what}: LLR bit patterns differ"


def _both_entries(dec, syn, want, what):
    _same(_device(dec, syn), want, what + ", device entry")
    _same(_host(dec, syn), want, what + ", host entry")


@pytest.fixture(scope="module")
def bb72_case(ldpc):
    """BB-72 H_X, uniform prior 0.06, 400 syndromes of errors at 0.06, 9 legs of [30, 20, ..., 20], gamma 0.125 in leg 0
    and uniform in (-0.24, 0.66) in the others; the model at stop_after 1 and 3, and plain min-sum."""
    H, _ = _bb72(ldpc)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 400, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    g = _gammas(9, 72)
    ref = {k: RelayModel(H, prior, g, NINE_LEGS, stop_after=k).decode(syn) for k in (1, 3)}
    plain = MinSumModel(H, prior, 30).decode(syn)
    q = weights_of(prior)
    # preconditions, on the model: lanes of one tile are in different legs; the relay converges what min-sum leaves;
    # stop_after = 3 returns a strictly lighter solution somewhere
    its, conv = ref[1][2], ref[1][1]
    assert ((conv == 1) & (its <= 30)).any() and ((conv == 1) & (its > 30)).any()
    assert ((plain[1] == 0) & (conv == 1)).any()
    w1, w3 = (ref[1][0] * q).sum(axis=1), (ref[3][0] * q).sum(axis=1)
    assert (w3 < w1).any() and not (w3 > w1).any() and np.array_equal(ref[1][1], ref[3][1])
    return H, syn, prior, g, ref


@pytest.mark.parametrize("stop_after", [1, 3])
@pytest.mark.parametrize("variant", [0, 2])
def test_bb72_nine_legs_equal_the_model_on_both_tiers_and_both_entries(ldpc, gpu, bb72_case, stop_after, variant):
    H, syn, prior, g, ref = bb72_case
    dec = _decoder(ldpc, H, prior, g, NINE_LEGS, stop_after=stop_after, kernel_variant=variant)
    assert dec.kernel == (2 if variant == 2 else 1) and dec.info().device == 0 and dec.info().kernel == dec.kernel
    assert dec.leg_iters.tolist() == NINE_LEGS and np.array_equal(dec.gammas, g)
    _both_entries(dec, syn, ref[stop_after], f"stop_after {stop_after}")
    assert len(dec.decode_batch_host(syn)) == 4 and dec.decode_batch_host(syn)[2] is None
    # the reference-style methods
    want = ref[stop_after]
    c = int(np.nonzero(want[2] > 30)[0][0])
    guess, ok = dec.decode_(syn[c])
    assert np.array_equal(guess, want[0][c]) and ok == bool(want[1][c])
    assert np.array_equal(dec.scratch.log_probabs, want[4][c].astype(np.float64))
    out = np.zeros((72, 400), dtype=np.uint8)
    _, success = dec.batchdecode_(syn.T, out)
    assert np.array_equal(out.T, want[0]) and np.array_equal(success, want[1].astype(bool))
    dec.close()


def test_default_gammas_are_those_of_the_seed(ldpc, gpu, bb72_case):
    """per=, seed=: the constructor's own gammas (leg 0 gamma0, the others uniform from default_rng(seed)) reach the device."""
    H, syn, prior, g, ref = bb72_case
    dec = ldpc.RelayMinSumDecoder(H, 0.06, 30, legs=9, leg_iters=20, seed=5)
    assert dec.per == 0.06 and np.array_equal(dec.gammas, g) and np.array_equal(dec.channel_llr.view(np.int32), prior.view(np.int32))
    _same(_device(dec, syn[:130]), tuple(x[:130] for x in ref[1]), "seed=5")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_short_legs_converged_and_unconverged_side_by_side(ldpc, gpu, bb72_case, variant):
    H, syn, prior, g, _ = bb72_case
    want = RelayModel(H, prior, g[:3], [4, 3, 3], stop_after=2).decode(syn[:130])
    assert 0 < want[1].sum() < 130 and set(want[3].tolist()) == {0, 1, 2}
    dec = _decoder(ldpc, H, prior, g[:3], [4, 3, 3], stop_after=2, kernel_variant=variant)
    _both_entries(dec, syn[:130], want, f"legs [4, 3, 3], tier {variant}")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_gamma_zero_and_one_leg_is_the_minsum_decoder(ldpc, gpu, bb72_case, variant):
    H, syn, prior, _, _ = bb72_case
    ms = MinSumModel(H, prior, 30).decode(syn[:200])
    assert 0 < ms[1].sum() < 200
    dec = _decoder(ldpc, H, prior, np.zeros((1, 72), dtype=np.float32), [30], kernel_variant=variant)
    got = _device(dec, syn[:200])
    _same(got, (ms[0], ms[1], ms[2], ms[1].astype(np.int32), ms[3]), "gamma 0 against the min-sum model")
    md = ldpc.MinSumDecoder(H, None, 30, channel_llr=prior, kernel_variant=variant)
    err, conv, llr, its = md.decode_batch_host(syn[:200], want_llr=True)
    assert np.array_equal(got[0], err) and np.array_equal(got[1], conv) and np.array_equal(got[3], its)
    assert np.array_equal(got[2].view(np.int64), llr.view(np.int64))
    dec.close(); md.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_per_bit_priors_on_240_8_4(ldpc, gpu, variant):
    """Per-bit priors in [1e-4, 0.45], three bits above 0.5 (negative prior LLR), negative gammas; batch 130 = two tiles
    of 64 and a ragged one (tier 2), eight tiles of 16 and a ragged one (tier 1)."""
    H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
    rng = np.random.default_rng(11)
    probs = rng.uniform(1e-4, 0.45, 240)
    probs[[3, 77, 200]] = [0.6, 0.75, 0.9]
    e = (rng.random((130, 240)) < np.minimum(probs, 0.04)[None, :]).astype(np.uint8)
    syn = ldpc.codes.syndromes_of(H, e)
    g = _gammas(3, 240, seed=2)
    assert (g < 0).any() and (g > 0).any()
    prior = llr_of_probs(probs)
    want = RelayModel(H, prior, g, [8, 6, 6], stop_after=2).decode(syn)
    assert 0 < want[1].sum() and len(set(want[2].tolist())) > 3
    dec = ldpc.RelayMinSumDecoder(H, None, 8, channel_probs=probs, legs=3, leg_iters=6, gammas=g, stop_after=2, kernel_variant=variant)
    assert dec.kernel == variant and dec.per is None and (dec.channel_llr < 0).sum() == 3
    _both_entries(dec, syn, want, f"tier {variant}")
    dec.close()


def _irregular():
    """150 bits, 27 checks: check 0 empty, check 1 of degree 1, checks 2 / 3 / 4 of degree 33 / 64 / 70, 22 random checks
    of degree 3..6 over bits 0..147; bit 148 sits in check 5 only, bit 149 in none (its prior is negative)."""
    rng = np.random.default_rng(21)
    Hd = np.zeros((27, 150), dtype=np.uint8)
    Hd[1, 5] = 1
    Hd[2, 10:43] = 1
    Hd[3, 20:84] = 1
    Hd[4, 60:130] = 1
    for i in range(5, 27):
        Hd[i, rng.choice(148, size=int(rng.integers(3, 7)), replace=False)] = 1
    Hd[5, 148] = 1
    deg = Hd.sum(axis=1)
    assert deg[0] == 0 and deg[1] == 1 and (deg[2], deg[3], deg[4]) == (33, 64, 70) and Hd[:, 148].sum() == 1 and Hd[:, 149].sum() == 0
    probs = rng.uniform(0.01, 0.3, 150)
    prior = llr_of_probs(probs)
    prior[149] = np.float32(-0.8)
    prior[7] = np.float32(1e-40)      # a subnormal prior: products with it stay subnormal, and are kept
    e = (rng.random((65, 150)) < 0.04).astype(np.uint8)
    syn = ((Hd.astype(np.int64) @ e.T.astype(np.int64)) % 2).T.astype(np.uint8)
    syn[40:, :] = rng.integers(0, 2, size=(25, 27))   # arbitrary syndromes; some set the empty check's entry
    assert syn[:, 0].any() and not syn[:40, 0].any()
    return sp.csc_matrix(Hd), prior, syn


def test_irregular_graph_every_record_form(ldpc, gpu):
    H, prior, syn = _irregular()
    g = _gammas(3, 150, seed=8)
    want = RelayModel(H, prior, g, [10, 6, 6], stop_after=2).decode(syn)
    assert want[1].any() and not want[1].all() and want[0][:, 149].all() and (want[2] > 10).any()
    ran = []
    for variant in (1, 2):
        try:
            dec = _decoder(ldpc, H, prior, g, [10, 6, 6], stop_after=2, kernel_variant=variant)
        except ldpc.LdpcError as e:
            assert variant == 1 and e.status == UNSUPPORTED
            continue
        assert dec.kernel == variant
        _both_entries(dec, syn, want, f"tier {variant}")
        ran.append(variant)
        dec.close()
    assert 2 in ran


def test_clamps_engage(ldpc, gpu, bb72_case):
    H, _, prior, g, _ = bb72_case
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 64, 0.06, seed=9))
    want = RelayModel(H, prior, g[:3], [30, 10, 10], alpha=1.0, clip=8.0).decode(syn)
    free = RelayModel(H, prior, g[:3], [30, 10, 10], alpha=1.0, clip=1e6).decode(syn)
    assert (want[4].view(np.int32) != free[4].view(np.int32)).any()      # the clamp changes this input's outcome
    for variant in (1, 2):
        dec = _decoder(ldpc, H, prior, g[:3], [30, 10, 10], alpha=1.0, clip=8.0, kernel_variant=variant)
        _same(_device(dec, syn), want, f"clip 8, tier {variant}")
        dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_a_handle_used_three_times_and_every_combination_of_optional_outputs(ldpc, gpu, bb72_case, variant):
    H, syn, prior, g, ref = bb72_case
    dec = _decoder(ldpc, H, prior, g, NINE_LEGS, stop_after=3, kernel_variant=variant)
    for lo, hi in ((150, 151), (0, 129), (399, 400)):
        want = tuple(x[lo:hi] for x in ref[3])
        _same(_device(dec, syn[lo:hi]), want, f"columns {lo}:{hi}")
    want = tuple(x[:129] for x in ref[3])
    for mask in range(8):
        kw = dict(want_llr=bool(mask & 1), want_iters=bool(mask & 2), want_sol=bool(mask & 4))
        _same(_device(dec, syn[:129], **kw), want, str(kw))
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_wide_syndrome_entries_and_legs_of_zero_iterations(ldpc, gpu, bb72_case, variant):
    H, syn, prior, g, _ = bb72_case
    syn = syn[:70]
    # an entry that is not 0 counts as 1
    want = RelayModel(H, prior, g[:3], [6, 4, 4], stop_after=2).decode(syn)
    dec = _decoder(ldpc, H, prior, g[:3], [6, 4, 4], stop_after=2, kernel_variant=variant)
    wide = syn.copy()
    wide[wide == 1] = np.where(np.arange((wide == 1).sum()) % 2 == 0, 2, 3)
    wide[0, np.nonzero(syn[0] == 0)[0][:2]] = [255, 128]
    plain = (wide != 0).astype(np.uint8)
    wide_want = RelayModel(H, prior, g[:3], [6, 4, 4], stop_after=2).decode(plain)
    _same(_device(dec, wide), wide_want, "entries 2, 3, 128, 255")
    _same(_device(dec, plain), wide_want, "entries 1")
    _same(_device(dec, syn), want, "the syndromes as they were")
    dec.close()
    # a leg of 0 iterations in the middle is skipped: [6, 0, 4] with three gamma rows is [6, 4] with rows 0 and 2
    gap = RelayModel(H, prior, g[:3], [6, 0, 4], stop_after=2).decode(syn)
    assert all(np.array_equal(a, b) for a, b in zip(gap, RelayModel(H, prior, g[[0, 2]], [6, 4], stop_after=2).decode(syn)))
    assert (gap[2] > 6).any() and not all(np.array_equal(a, b) for a, b in zip(gap, RelayModel(H, prior, g[:2], [6, 4], stop_after=2).decode(syn)))
    L = ldpc._capi.lib()
    import ctypes

    def handle(leg_iters):
        h = ctypes.c_void_p()
        o = ldpc._capi.RelayOptions()
        o.device, o.kernel_variant, o.stop_after = 0, variant, 2
        M = sp.csc_matrix(H)
        colptr, rowval = M.indptr.astype(np.int64), M.indices.astype(np.int64)
        its = np.asarray(leg_iters, dtype=np.int32)
        g3 = np.ascontiguousarray(g[:3])
        assert L.ldpc_relay_create(36, 72, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, prior.ctypes.data, 3,
                                   g3.ctypes.data, its.ctypes.data, ctypes.byref(o), ctypes.byref(h)) == 0, L.ldpc_last_error()
        return h

    def run(h):
        err = np.full((70, 72), 7, dtype=np.uint8)
        conv = np.full(70, 7, dtype=np.uint8)
        llr = np.full((70, 72), 7.0)
        its, sol = np.full(70, -7, dtype=np.int32), np.full(70, -7, dtype=np.int32)
        s8 = np.ascontiguousarray(syn)
        assert L.ldpc_relay_decode_batch(h, 70, s8.ctypes.data, err.ctypes.data, conv.ctypes.data, llr.ctypes.data,
                                         its.ctypes.data, sol.ctypes.data) == 0, L.ldpc_last_error()
        assert L.ldpc_relay_decode_batch(h, 0, None, None, None, None, None, None) == 0    # batch 0: nothing touched
        assert L.ldpc_relay_destroy(h) == 0
        return err, conv, llr, its, sol

    _same(run(handle([6, 0, 4])), gap, "leg_iters [6, 0, 4]")
    # every leg of 0 iterations: zeros, exactly as max_iters = 0 of min-sum
    err, conv, llr, its, sol = run(handle([0, 0, 0]))
    assert not err.any() and not conv.any() and not its.any() and not sol.any() and not llr.view(np.int64).any()


def test_a_tie_keeps_the_earlier_solution_and_the_llrs_are_the_last_ones(ldpc, gpu):
    """Four bits, equal priors: (0, 0, 1, 0) and then (0, 0, 0, 1) of the same weight are found; the first one stays.
    One syndrome in a tile of 64 (63 idle lanes), and 70 copies of it."""
    H = np.array([[1, 1, 0, 0], [0, 1, 1, 1]], dtype=np.uint8)
    g = np.array([[0.75, -0.625, 0.75, -0.375], [-0.125, 0.625, -0.125, 0.125], [-0.875, 0.5, 0.125, -0.25]], dtype=np.float32)
    prior = np.ones(4, dtype=np.float32)
    syn = np.tile(np.array([[0, 1]], dtype=np.uint8), (70, 1))
    syn[1::2] = [[1, 0]]
    want = RelayModel(H, prior, g, [3, 3, 3], alpha=1.0, stop_after=3).decode(syn)
    assert want[0][0].tolist() == [0, 0, 1, 0] and want[3][0] == 3 and (want[4][0] <= 0).astype(int).tolist() == [0, 0, 0, 1]
    for variant in (1, 2):
        dec = _decoder(ldpc, H, prior, g, [3, 3, 3], alpha=1.0, stop_after=3, kernel_variant=variant)
        _both_entries(dec, syn, want, f"tier {variant}")
        _same(_device(dec, syn[:1]), tuple(x[:1] for x in want), f"tier {variant}, one column")
        dec.close()


# ---- compositions: model sampler -> model decoder -> model score ---------------------------------------------------

SHORT = [12, 8, 8]


def _model_guesses(H, prior, g, syn):
    err, conv, _, _, _ = RelayModel(H, prior, g, SHORT).decode(syn)
    return err, int((conv == 0).sum())


def test_run_trials_equals_model_sampler_model_decoder_model_score(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    g = _gammas(3, 72)
    dec = ldpc.RelayMinSumDecoder(Hx, 0.03, 12, legs=3, leg_iters=8, gammas=g)
    res = ldpc.run_trials(dec, 1000, per=0.03, batch=256, seed=7, logicals=Lz)
    errors = tm.sample(72, 1000, 0.03, seed=7)
    guesses, nc = _model_guesses(Hx, llr_of_probs(np.full(72, 0.03)), g, tm.syndromes(Hx, errors))
    _, want = tm.score(Hx, Lz, guesses, errors)
    assert res == ldpc.TrialResult(1000, int(want[1]), int(want[2]), int(want[3]), nc)
    assert 0 < res.block_errors < 1000
    dec.close()


def test_run_css_trials_with_biased_marginals(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    px, py, pz = 0.01, 0.002, 0.03
    prior_x, prior_z = llr_of_probs(np.full(72, px + py)), llr_of_probs(np.full(72, py + pz))   # X parts / Z parts
    g = _gammas(3, 72)
    dec_hz = ldpc.RelayMinSumDecoder(Hz, None, 12, channel_probs=np.full(72, px + py), legs=3, leg_iters=8, gammas=g)
    dec_hx = ldpc.RelayMinSumDecoder(Hx, None, 12, channel_probs=np.full(72, py + pz), legs=3, leg_iters=8, gammas=g)
    res = ldpc.run_css_trials(dec_hx, dec_hz, 512, (px, py, pz), batch=200, seed=5, logicals=(Lx, Lz))
    ex, ez = cm.sample(72, 512, (px, py, pz), seed=5)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    gx, nc_hz = _model_guesses(Hz, prior_x, g, sz)
    gz, nc_hx = _model_guesses(Hx, prior_z, g, sx)
    _, want = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    assert res == ldpc.CSSTrialResult(512, int(want[1]), int(want[2]), int(want[3]), int(want[4]), int(want[5]), nc_hx, nc_hz)
    assert res.block_errors > 0
    dec_hx.close(); dec_hz.close()


def test_bposd_around_a_relay_decoder(ldpc, gpu):
    import torch

    H, _ = _bb72(ldpc)
    Hd = np.asarray(H.todense()).astype(np.uint8)
    e = np.concatenate([ldpc.codes.random_errors(72, 100, 0.03, seed=4), ldpc.codes.random_errors(72, 100, 0.08, seed=6)])
    syn = ldpc.codes.syndromes_of(H, e)
    g = _gammas(3, 72)
    prior = llr_of_probs(np.full(72, 0.03))
    merr, mconv, _, _, mM = RelayModel(H, prior, g, [4, 3, 3]).decode(syn)   # short legs: unconverged columns for the OSD step
    assert 0 < mconv.sum() < 200
    want = np.stack([osd_model_postprocess(Hd, syn[b], merr[b], mM[b].astype(np.float64), 2) for b in range(200)])
    relay = ldpc.RelayMinSumDecoder(H, 0.03, 4, legs=3, leg_iters=3, gammas=g)
    dec = ldpc.BeliefPropagationOSDDecoder(H, osd_order=2, osd="device", bp_decoder=relay)
    assert dec.bp_decoder is relay
    out, conv, k = dec.batchdecode_device(torch.from_numpy(syn).cuda())
    torch.cuda.synchronize()
    out, conv = out.cpu().numpy(), conv.cpu().numpy()
    assert k == 200 and np.array_equal(conv, mconv)
    assert np.array_equal(out, want), f"{int((out != want).any(axis=1).sum())} columns differ from the model chain"
    assert np.array_equal(ldpc.codes.syndromes_of(H, out), syn)      # every column reproduces its syndrome
    relay.close()
