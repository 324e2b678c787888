"""Min-sum decoder on the GPU against the numpy model of its rule (tests/minsum_model.py): equality in every element --
errors, flags, iteration counts, and the LLRs as bit patterns -- on the smallest shapes that reach every code path:
both tiers, tiles of 64 / 32 / 16 syndromes, ragged tiles, every record form (check degree <= 32, <= 64, per edge),
empty and degree-1 nodes, the clamps, and the compositions with the trials loops and the OSD step."""
import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import trials_model as tm
from minsum_model import MinSumModel, llr_of_probs
from osd_model import osd_model_postprocess

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5


def _bb72(ldpc):
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx, dtype=np.uint8)), sp.csc_matrix(np.asarray(Hz, dtype=np.uint8))


def _device(dec, syn, want_llr=True, want_iters=True):
    import torch

    B = syn.shape[0]
    d_syn = torch.from_numpy(np.ascontiguousarray(syn, dtype=np.uint8)).cuda()
    err = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    dec.decode_batch_device(d_syn, err, conv, llr, its)
    torch.cuda.synchronize()
    return (err.cpu().numpy(), conv.cpu().numpy(), llr.cpu().numpy() if want_llr else None,
            its.cpu().numpy() if want_iters else None)


def _same(got, want, what=""):
    """got = (err, conv, llr f64 | None, iters | None) of the library, want = (err, conv, iters, L f32) of the model."""
    err, conv, llr, its = got
    merr, mconv, mits, mL = want
    assert np.array_equal(err, merr), f"{what}: errors differ in {int((err != merr).any(axis=1).sum())} columns"
    assert np.array_equal(conv, mconv), f"{what}: converged flags differ"
    if its is not None:
        assert np.array_equal(its, mits), f"{what}: iteration counts differ"
    if llr is not None:
        assert llr.dtype == np.float64
        assert np.array_equal(llr.view(np.int64), mL.astype(np.float64).view(np.int64)), f"{what}: LLR bit patterns differ"


@pytest.fixture(scope="module")
def bb72_case(ldpc):
    """BB-72 H_X, uniform prior 0.03; 200 syndromes of errors sampled at 0.01 / 0.03 / 0.06; the model at alpha 0.75, 1."""
    H, _ = _bb72(ldpc)
    e = np.concatenate([ldpc.codes.random_errors(72, 66, 0.01, seed=1), ldpc.codes.random_errors(72, 67, 0.03, seed=2),
                        ldpc.codes.random_errors(72, 67, 0.06, seed=3)])
    syn = ldpc.codes.syndromes_of(H, e)
    prior = llr_of_probs(np.full(72, 0.03))
    ref = {a: MinSumModel(H, prior, 30, alpha=a).decode(syn) for a in (0.75, 1.0)}
    assert 0 < ref[0.75][1].sum() < 200 and len(set(ref[0.75][2].tolist())) > 3   # converged and not, many iteration counts
    return H, syn, ref


@pytest.mark.parametrize("alpha", [0.75, 1.0])
@pytest.mark.parametrize("variant", [0, 2])
def test_bb72_equals_the_model_on_both_tiers_and_both_entries(ldpc, gpu, bb72_case, alpha, variant):
    H, syn, ref = bb72_case
    dec = ldpc.MinSumDecoder(H, 0.03, 30, alpha=alpha, kernel_variant=variant)
    assert dec.kernel == (2 if variant == 2 else 1) and dec.per == 0.03 and dec.info().device == 0
    assert np.array_equal(dec.channel_llr.view(np.int32), llr_of_probs(np.full(72, 0.03)).view(np.int32))
    _same(_device(dec, syn), ref[alpha], "device entry")
    err, conv, llr, its = dec.decode_batch_host(syn, want_llr=True)
    _same((err, conv, llr, its), ref[alpha], "host entry")
    assert dec.decode_batch_host(syn)[2] is None
    # the reference-style methods
    guess, ok = dec.decode_(syn[5])
    assert np.array_equal(guess, ref[alpha][0][5]) and ok == bool(ref[alpha][1][5])
    assert np.array_equal(dec.scratch.log_probabs, ref[alpha][3][5].astype(np.float64))
    out = np.zeros((72, 200), dtype=np.uint8)
    _, success = dec.batchdecode_(syn.T, out)
    assert np.array_equal(out.T, ref[alpha][0]) and np.array_equal(success, ref[alpha][1].astype(bool))
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_per_bit_priors_on_240_8_4(ldpc, gpu, variant):
    """Per-bit priors in [1e-4, 0.45], a few bits above 0.5 (negative prior LLR); batch 130 = two tiles of 64 and a
    ragged one (tier 2), eight tiles of 16 and a ragged one (tier 1)."""
    H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
    rng = np.random.default_rng(11)
    probs = rng.uniform(1e-4, 0.45, 240)
    probs[[3, 77, 200]] = [0.6, 0.75, 0.9]
    e = (rng.random((130, 240)) < np.minimum(probs, 0.04)[None, :]).astype(np.uint8)
    syn = ldpc.codes.syndromes_of(H, e)
    want = MinSumModel(H, llr_of_probs(probs), 20).decode(syn)
    dec = ldpc.MinSumDecoder(H, None, 20, channel_probs=probs, kernel_variant=variant)
    assert dec.kernel == variant and dec.per is None and (dec.channel_llr < 0).sum() == 3
    _same(_device(dec, syn), want, f"tier {variant}")
    dec.close()
    dec = ldpc.MinSumDecoder(H, None, 20, channel_llr=llr_of_probs(probs), kernel_variant=variant)
    _same(_device(dec, syn), want, f"tier {variant}, channel_llr=")
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
    prior[7] = np.float32(1e-40)      # a subnormal prior: alpha * |b| stays subnormal, and is kept
    prior[8] = np.float32(-0.0)
    e = (rng.random((65, 150)) < 0.04).astype(np.uint8)
    syn = ((Hd.astype(np.int64) @ e.T.astype(np.int64)) % 2).T.astype(np.uint8)
    syn[40:, :] = rng.integers(0, 2, size=(25, 27))   # arbitrary syndromes; some set the empty check's entry
    assert syn[:, 0].any() and not syn[:40, 0].any()
    return sp.csc_matrix(Hd), prior, syn


def test_irregular_graph_every_record_form(ldpc, gpu):
    H, prior, syn = _irregular()
    want = MinSumModel(H, prior, 20).decode(syn)
    assert want[1].any() and not want[1].all() and want[0][:, 149].all()
    ran = []
    for variant in (1, 2):
        try:
            dec = ldpc.MinSumDecoder(H, None, 20, channel_llr=prior, kernel_variant=variant)
        except ldpc.LdpcError as e:
            assert variant == 1 and e.status == UNSUPPORTED
            continue
        assert dec.kernel == variant
        _same(_device(dec, syn), want, f"tier {variant}")
        ran.append(variant)
        dec.close()
    assert 2 in ran


def test_clamps_engage(ldpc, gpu):
    H, _ = _bb72(ldpc)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 64, 0.06, seed=9))
    prior = llr_of_probs(np.full(72, 0.06))
    want = MinSumModel(H, prior, 50, alpha=1.0, clip=8.0).decode(syn)
    free = MinSumModel(H, prior, 50, alpha=1.0, clip=1e6).decode(syn)
    assert (want[3].view(np.int32) != free[3].view(np.int32)).any()      # the clamp changes this input's outcome
    for variant in (1, 2):
        dec = ldpc.MinSumDecoder(H, 0.06, 50, alpha=1.0, clip=8.0, kernel_variant=variant)
        _same(_device(dec, syn), want, f"clip 8, tier {variant}")
        dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_max_iters_zero_and_one_and_wide_syndrome_entries(ldpc, gpu, bb72_case, variant):
    H, syn, _ = bb72_case
    prior = llr_of_probs(np.full(72, 0.03))
    dec = ldpc.MinSumDecoder(H, 0.03, 0, kernel_variant=variant)
    err, conv, llr, its = _device(dec, syn[:70])
    assert not err.any() and not conv.any() and not its.any() and not llr.view(np.int64).any()
    err, conv, llr, its = dec.decode_batch_host(syn[:70], want_llr=True)
    assert not err.any() and not conv.any() and not its.any() and not llr.view(np.int64).any()
    dec.close()
    dec = ldpc.MinSumDecoder(H, 0.03, 1, kernel_variant=variant)
    want = MinSumModel(H, prior, 1).decode(syn[:70])
    assert want[1].any() and not want[1].all()
    _same(_device(dec, syn[:70]), want, "max_iters 1")
    dec.close()
    # an entry that is not 0 counts as 1
    dec = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant)
    wide = syn[:70].copy()
    wide[wide == 1] = np.where(np.arange((wide == 1).sum()) % 2 == 0, 2, 3)
    wide[0, np.nonzero(syn[0] == 0)[0][:2]] = [255, 128]
    plain = (wide != 0).astype(np.uint8)
    want = MinSumModel(H, prior, 30).decode(plain)
    _same(_device(dec, wide), want, "entries 2, 3, 128, 255")
    _same(_device(dec, plain), want, "entries 1")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_a_handle_used_twice_and_optional_outputs(ldpc, gpu, bb72_case, variant):
    H, syn, ref = bb72_case
    dec = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant)
    for lo, hi in ((150, 151), (0, 129), (199, 200)):
        want = tuple(x[lo:hi] for x in ref[0.75])
        _same(_device(dec, syn[lo:hi]), want, f"columns {lo}:{hi}")
    want = tuple(x[:129] for x in ref[0.75])
    _same(_device(dec, syn[:129], want_llr=False, want_iters=False), want, "llr=None, iters=None")
    _same(_device(dec, syn[:129], want_llr=True, want_iters=False), want, "iters=None")
    _same(_device(dec, syn[:129], want_llr=False, want_iters=True), want, "llr=None")
    dec.close()


def _model_guesses(H, prior, max_iters, syn):
    err, conv, _, _ = MinSumModel(H, prior, max_iters).decode(syn)
    return err, int((conv == 0).sum())


def test_run_trials_equals_model_sampler_model_decoder_model_score(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    dec = ldpc.MinSumDecoder(Hx, 0.03, 30)
    res = ldpc.run_trials(dec, 1000, per=0.03, batch=256, seed=7, logicals=Lz)
    errors = tm.sample(72, 1000, 0.03, seed=7)
    guesses, nc = _model_guesses(Hx, llr_of_probs(np.full(72, 0.03)), 30, tm.syndromes(Hx, errors))
    _, want = tm.score(Hx, Lz, guesses, errors)
    assert res == ldpc.TrialResult(1000, int(want[1]), int(want[2]), int(want[3]), nc)
    assert 0 < res.block_errors < 1000
    dec.close()


def test_run_css_trials_with_biased_marginals(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    px, py, pz = 0.01, 0.002, 0.03
    prior_x, prior_z = llr_of_probs(np.full(72, px + py)), llr_of_probs(np.full(72, py + pz))   # X parts / Z parts
    dec_hz = ldpc.MinSumDecoder(Hz, None, 30, channel_probs=np.full(72, px + py))   # decodes sz = Hz ex: guesses the X parts
    dec_hx = ldpc.MinSumDecoder(Hx, None, 30, channel_probs=np.full(72, py + pz))   # decodes sx = Hx ez: guesses the Z parts
    res = ldpc.run_css_trials(dec_hx, dec_hz, 512, (px, py, pz), batch=200, seed=5, logicals=(Lx, Lz))
    ex, ez = cm.sample(72, 512, (px, py, pz), seed=5)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    gx, nc_hz = _model_guesses(Hz, prior_x, 30, sz)
    gz, nc_hx = _model_guesses(Hx, prior_z, 30, sx)
    _, want = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    assert res == ldpc.CSSTrialResult(512, int(want[1]), int(want[2]), int(want[3]), int(want[4]), int(want[5]), nc_hx, nc_hz)
    assert res.block_errors > 0
    dec_hx.close(); dec_hz.close()


def test_bposd_around_a_minsum_decoder(ldpc, gpu):
    import torch

    H, _ = _bb72(ldpc)
    Hd = np.asarray(H.todense()).astype(np.uint8)
    e = np.concatenate([ldpc.codes.random_errors(72, 100, 0.03, seed=4), ldpc.codes.random_errors(72, 100, 0.08, seed=6)])
    syn = ldpc.codes.syndromes_of(H, e)
    merr, mconv, _, mL = MinSumModel(H, llr_of_probs(np.full(72, 0.03)), 30).decode(syn)
    assert 0 < mconv.sum() < 200
    want = np.stack([osd_model_postprocess(Hd, syn[b], merr[b], mL[b].astype(np.float64), 2) for b in range(200)])
    ms = ldpc.MinSumDecoder(H, 0.03, 30)
    dec = ldpc.BeliefPropagationOSDDecoder(H, osd_order=2, osd="device", bp_decoder=ms)
    assert dec.bp_decoder is ms
    out, conv, k = dec.batchdecode_device(torch.from_numpy(syn).cuda())
    torch.cuda.synchronize()
    out, conv = out.cpu().numpy(), conv.cpu().numpy()
    assert k == 200 and np.array_equal(conv, mconv)
    assert np.array_equal(out, want), f"{int((out != want).any(axis=1).sum())} columns differ from the model chain"
    assert np.array_equal(ldpc.codes.syndromes_of(H, out), syn)      # every column reproduces its syndrome
    # the host form of the OSD step on the same input
    host = ldpc.BeliefPropagationOSDDecoder(H, osd_order=2, osd="host", bp_decoder=ms)
    out, conv, k = host.batchdecode_device(torch.from_numpy(syn).cuda())
    assert k == 200 and np.array_equal(conv.cpu().numpy(), mconv)
    assert np.array_equal(ldpc.codes.syndromes_of(H, out.cpu().numpy()), syn)
    errors = np.zeros((72, 200), dtype=np.uint8)
    _, success = host.batchdecode_(syn.T, errors)
    assert np.array_equal(ldpc.codes.syndromes_of(H, np.ascontiguousarray(errors.T)), syn) and np.array_equal(success, mconv.astype(bool))
    guess, ok = host.decode_(syn[3])
    assert np.array_equal(ldpc.codes.syndromes_of(H, guess[None, :].astype(np.uint8))[0], syn[3]) and ok == bool(mconv[3])
    ms.close()
