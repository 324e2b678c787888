"""Guided-decimation min-sum decoder on the GPU against the numpy model of its rule (tests/decim_model.py): equality in
every element -- errors, flags, iteration counts, decimation counts, and the LLRs as bit patterns -- on both tiers, through
the device entry and the host entry, on the smallest shapes that reach every code path: lanes of one tile that stop in
round 0, after a decimation, and with every bit pinned; tiles of 64 / 16 syndromes, ragged tiles, a partial last word of
D, every record form, the clamp, a tile after another in one slot, and the compositions with the trials loop and the OSD
step.  Every case asserts on the model first that it holds what it is there for."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import trials_model as tm
from decim_model import DecimModel
from minsum_model import MinSumModel, llr_of_probs
from osd_model import osd_model_postprocess

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5


def _bb72(ldpc):
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx, dtype=np.uint8)), sp.csc_matrix(np.asarray(Hz, dtype=np.uint8))


def _decoder(ldpc, H, prior, T, Dmax, **kw):
    return ldpc.DecimatedMinSumDecoder(H, None, T, channel_llr=prior, max_decimations=Dmax, **kw)


def _device(dec, syn, want_llr=True, want_iters=True, want_dec=True):
    import torch

    B = syn.shape[0]
    d_syn = torch.from_numpy(np.ascontiguousarray(syn, dtype=np.uint8)).cuda()
    err = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    ndec = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_dec else None
    dec.decode_batch_device(d_syn, err, conv, llr, its, ndec)
    torch.cuda.synchronize()
    return (err.cpu().numpy(), conv.cpu().numpy(), llr.cpu().numpy() if want_llr else None,
            its.cpu().numpy() if want_iters else None, ndec.cpu().numpy() if want_dec else None)


def _host(dec, syn):
    return dec.decode_batch_host(syn, want_llr=True, want_decimated=True)


def _same(got, want, what=""):
    """got = (err, conv, llr f64 | None, iters | None, decimated | None) of the library, want = (err, conv, iters,
    decimated, L f32) of the model."""
    err, conv, llr, its, ndec = got
    merr, mconv, mits, mdec, mL = want
    assert err.dtype == np.uint8 and conv.dtype == np.uint8
    assert np.array_equal(err, merr), f"{what}: errors differ in {int((err != merr).any(axis=1).sum())} columns"
    assert np.array_equal(conv, mconv), f"{what}: converged flags differ"
    if its is not None:
        assert its.dtype == np.int32 and np.array_equal(its, mits), f"{what}: iteration counts differ"
    if ndec is not None:
        assert ndec.dtype == np.int32 and np.array_equal(ndec, mdec), f"{what}: decimation counts differ"
    if llr is not None:
        assert llr.dtype == np.float64
        assert np.array_equal(llr.view(np.int64), mL.astype(np.float64).view(np.int64)), f"{what}: LLR bit patterns differ"


def _both_entries(dec, syn, want, what):
    _same(_device(dec, syn), want, what + ", device entry")
    _same(_host(dec, syn), want, what + ", host entry")


def _rows(want, sel):
    return tuple(x[sel] for x in want)


@pytest.fixture(scope="module")
def bb72_case(ldpc):
    """BB-72 H_X, uniform prior 0.06, the 400 syndromes of errors at 0.06 of seed 3; the model with rounds of 5 and every
    bit free to be pinned on the first 130 (two full tiles and a ragged one), and with rounds of 3 and at most 6
    decimations on all 400."""
    H, _ = _bb72(ldpc)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 400, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    main = DecimModel(H, prior, 5, 72).decode(syn[:130])
    short = DecimModel(H, prior, 3, 6).decode(syn)
    # preconditions, on the model.  Main: lanes of one tile stop in round 0 and after decimations; two columns end with
    # every bit pinned (the |D| == n exit)
    err, conv, its, ndec, L = main
    assert int(conv.sum()) == 128 and int(((conv == 1) & (ndec == 0)).sum()) == 68 and int(((conv == 1) & (ndec > 0)).sum()) == 60
    assert int(((conv == 0) & (ndec == 72)).sum()) == 2 == int((conv == 0).sum())
    assert int(((conv[:64] == 1) & (ndec[:64] > 0)).sum()) == 26 and ((conv[:64] == 1) & (ndec[:64] == 0)).any()
    assert int(its.max()) == 365 and (np.abs(L[conv == 0]) == np.float32(2e6)).all()
    # short rounds, first 130: every decimation count occurs, converged and given-up lanes side by side
    err, conv, its, ndec, L = _rows(short, slice(0, 130))
    assert int(conv.sum()) == 100 and int(((conv == 1) & (ndec == 0)).sum()) == 50 and int(((conv == 1) & (ndec > 0)).sum()) == 50
    assert int((conv == 0).sum()) == 30 and set(ndec.tolist()) == set(range(7)) and int(its.max()) == 21
    return H, syn, prior, main, short


@pytest.mark.parametrize("variant", [0, 2])
def test_bb72_equals_the_model_on_both_tiers_and_both_entries(ldpc, gpu, bb72_case, variant):
    H, syn, prior, main, _ = bb72_case
    dec = _decoder(ldpc, H, prior, 5, 72, kernel_variant=variant)
    info = dec.info()
    assert dec.kernel == (2 if variant == 2 else 1) and info.device == 0 and info.kernel == dec.kernel
    assert info.tile_syndromes == 64 and info.last_grid == 0
    _both_entries(dec, syn[:130], main, f"T 5, Dmax 72, tier {dec.kernel}")
    assert dec.info().last_grid == 3
    assert len(dec.decode_batch_host(syn[:130])) == 4 and dec.decode_batch_host(syn[:130])[2] is None
    # the reference-style methods, on a column that was rescued by decimations
    c = int(np.nonzero((main[1] == 1) & (main[3] > 0))[0][0])
    guess, ok = dec.decode_(syn[c])
    assert np.array_equal(guess, main[0][c]) and ok is True
    assert np.array_equal(dec.scratch.log_probabs, main[4][c].astype(np.float64))
    out = np.zeros((72, 130), dtype=np.uint8)
    _, success = dec.batchdecode_(syn[:130].T, out)
    assert np.array_equal(out.T, main[0]) and np.array_equal(success, main[1].astype(bool))
    dec.close()


def test_the_constructor_defaults_are_rounds_of_ten_and_every_bit(ldpc, gpu, bb72_case):
    """per=, no max_decimations: 10 iterations a round, up to n decimations reach the device."""
    H, syn, prior, _, _ = bb72_case
    dec = ldpc.DecimatedMinSumDecoder(H, 0.06)
    assert (dec.max_iters, dec.max_decimations, dec.per) == (10, 72, 0.06)
    assert np.array_equal(dec.channel_llr.view(np.int32), prior.view(np.int32))
    want = DecimModel(H, prior, 10, 72).decode(syn[:64])
    assert 0 < ((want[1] == 1) & (want[3] > 0)).sum()
    _same(_device(dec, syn[:64]), want, "the defaults")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_short_rounds_optional_outputs_slices_wide_entries_and_the_empty_calls(ldpc, gpu, bb72_case, variant):
    H, syn, prior, _, short = bb72_case
    dec = _decoder(ldpc, H, prior, 3, 6, kernel_variant=variant)
    assert dec.kernel == variant
    _both_entries(dec, syn[:130], _rows(short, slice(0, 130)), f"T 3, Dmax 6, tier {variant}")
    # every combination of the optional outputs
    for mask in range(8):
        kw = dict(want_llr=bool(mask & 1), want_iters=bool(mask & 2), want_dec=bool(mask & 4))
        _same(_device(dec, syn[:130], **kw), _rows(short, slice(0, 130)), str(kw))
    # one handle, three calls on slices
    for lo, hi in ((150, 151), (0, 129), (399, 400)):
        _same(_device(dec, syn[lo:hi]), _rows(short, slice(lo, hi)), f"columns {lo}:{hi}")
    # an entry that is not 0 counts as 1
    part = syn[:70]
    wide = part.copy()
    wide[wide == 1] = np.where(np.arange((wide == 1).sum()) % 2 == 0, 2, 3)
    wide[0, np.nonzero(part[0] == 0)[0][:2]] = [255, 128]
    plain = (wide != 0).astype(np.uint8)
    assert (plain != part).any()
    wide_want = DecimModel(H, prior, 3, 6).decode(plain)
    _same(_device(dec, wide), wide_want, "entries 2, 3, 128, 255")
    _same(_device(dec, plain), wide_want, "entries 1")
    _same(_device(dec, part), _rows(short, slice(0, 70)), "the syndromes as they were")
    dec.close()
    # the raw C entry: round_iters = 0 gives zeros everywhere; batch = 0 touches nothing
    L = ldpc._capi.lib()
    M = sp.csc_matrix(H)
    colptr, rowval = M.indptr.astype(np.int64), M.indices.astype(np.int64)
    for T in (0, 3):
        h = ctypes.c_void_p()
        o = ldpc._capi.DecimOptions()
        o.device, o.kernel_variant = 0, variant
        assert L.ldpc_decim_create(36, 72, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, prior.ctypes.data, T, 6,
                                   ctypes.byref(o), ctypes.byref(h)) == 0, L.ldpc_last_error()
        err = np.full((70, 72), 7, dtype=np.uint8)
        conv = np.full(70, 7, dtype=np.uint8)
        llr = np.full((70, 72), 7.0)
        its, ndec = np.full(70, -7, dtype=np.int32), np.full(70, -7, dtype=np.int32)
        s8 = np.ascontiguousarray(part)
        assert L.ldpc_decim_decode_batch(h, 0, None, None, None, None, None, None) == 0      # batch 0: LDPC_OK ...
        assert L.ldpc_decim_decode_batch(h, 0, s8.ctypes.data, err.ctypes.data, conv.ctypes.data, llr.ctypes.data,
                                         its.ctypes.data, ndec.ctypes.data) == 0
        assert (err == 7).all() and (conv == 7).all() and (llr == 7.0).all() and (its == -7).all() and (ndec == -7).all()   # ... nothing touched
        assert L.ldpc_decim_decode_batch_device(h, 0, None, None, None, None, None, None, None) == 0
        assert L.ldpc_decim_last_grid(h) == 0
        assert L.ldpc_decim_decode_batch(h, 70, s8.ctypes.data, err.ctypes.data, conv.ctypes.data, llr.ctypes.data,
                                         its.ctypes.data, ndec.ctypes.data) == 0, L.ldpc_last_error()
        assert L.ldpc_decim_destroy(h) == 0
        if T == 0:
            assert not err.any() and not conv.any() and not its.any() and not ndec.any() and not llr.view(np.int64).any()
        else:
            _same((err, conv, llr, its, ndec), _rows(short, slice(0, 70)), "the raw C entry")


@pytest.mark.parametrize("variant", [1, 2])
def test_no_decimation_is_the_minsum_decoder(ldpc, gpu, bb72_case, variant):
    H, syn, prior, _, _ = bb72_case
    ms = MinSumModel(H, prior, 30).decode(syn[:200])
    assert 0 < ms[1].sum() < 200
    dec = _decoder(ldpc, H, prior, 30, 0, kernel_variant=variant)
    got = _device(dec, syn[:200])
    _same(got, (ms[0], ms[1], ms[2], np.zeros(200, dtype=np.int32), ms[3]), "Dmax 0 against the min-sum model")
    _same(_host(dec, syn[:200]), (ms[0], ms[1], ms[2], np.zeros(200, dtype=np.int32), ms[3]), "Dmax 0 against the min-sum model, host entry")
    md = ldpc.MinSumDecoder(H, None, 30, channel_llr=prior, kernel_variant=variant)
    err, conv, llr, its = md.decode_batch_host(syn[:200], want_llr=True)
    assert np.array_equal(got[0], err) and np.array_equal(got[1], conv) and np.array_equal(got[3], its)
    assert np.array_equal(got[2].view(np.int64), llr.view(np.int64))
    dec.close(); md.close()


def test_the_hand_checked_case_on_the_device(ldpc, gpu):
    """One check over two bits, syndrome 1, equal priors (tests/test_decim_cpu.py walks through it): one column in a tile of
    64, then 70 copies alternating with syndrome 0 (which converges at once).  n = 2: a single, partial word of D."""
    H = np.array([[1, 1]], dtype=np.uint8)
    prior = np.ones(2, dtype=np.float32)
    syn = np.zeros((70, 1), dtype=np.uint8)
    syn[0::2] = 1
    want = DecimModel(H, prior, 2, 2, alpha=1.0).decode(syn)
    assert [x[0].tolist() for x in want] == [[1, 0], 1, 4, 1, [-2000000.0, 1000001.0]]
    assert [x[1].tolist() for x in want] == [[0, 0], 1, 1, 0, [2.0, 2.0]]
    assert MinSumModel(H, prior, 50, alpha=1.0).decode(syn[:1])[1][0] == 0
    for variant in (1, 2):
        dec = _decoder(ldpc, H, prior, 2, 2, alpha=1.0, kernel_variant=variant)
        assert dec.kernel == variant and dec.info().tile_syndromes == 64
        _same(_device(dec, syn[:1]), _rows(want, slice(0, 1)), f"tier {variant}, one column")
        _both_entries(dec, syn, want, f"tier {variant}")
        dec.close()


def _c240(ldpc):
    """The inputs of test_per_bit_priors_on_240_8_4 of the relay tests: per-bit priors in [1e-4, 0.45], three bits above 0.5."""
    H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
    rng = np.random.default_rng(11)
    probs = rng.uniform(1e-4, 0.45, 240)
    probs[[3, 77, 200]] = [0.6, 0.75, 0.9]
    e = (rng.random((130, 240)) < np.minimum(probs, 0.04)[None, :]).astype(np.uint8)
    return H, probs, ldpc.codes.syndromes_of(H, e)


@pytest.mark.parametrize("variant", [1, 2])
def test_per_bit_priors_on_240_8_4(ldpc, gpu, variant):
    """Batch 130 = eight tiles of 16 and a ragged one (tier 1: 3032 bytes a lane), two tiles of 64 and a ragged one (tier 2)."""
    H, probs, syn = _c240(ldpc)
    prior = llr_of_probs(probs)
    want = DecimModel(H, prior, 4, 12).decode(syn)
    err, conv, its, ndec, L = want
    assert int(conv.sum()) == 59 and int(((conv == 1) & (ndec > 0)).sum()) == 44 and int(((conv == 0) & (ndec == 12)).sum()) == 71
    assert len(set(its.tolist())) == 22
    dec = ldpc.DecimatedMinSumDecoder(H, None, 4, channel_probs=probs, max_decimations=12, kernel_variant=variant)
    assert dec.kernel == variant and dec.per is None and (dec.channel_llr < 0).sum() == 3
    assert dec.info().tile_syndromes == (16 if variant == 1 else 64)
    _both_entries(dec, syn, want, f"tier {variant}")
    assert dec.info().last_grid == (9 if variant == 1 else 3)
    dec.close()


def _irregular():
    """The irregular graph of the relay tests, by the same recipe.  150 bits, 27 checks: check 0 empty, check 1 of degree 1,
    checks 2 / 3 / 4 of degree 33 / 64 / 70, 22 random checks of degree 3..6 over bits 0..147; bit 148 sits in check 5 only,
    bit 149 in none (its prior is negative).  n = 150 leaves the last word of D partial."""
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
    prior[7] = np.float32(1e-40)      # a subnormal prior
    e = (rng.random((65, 150)) < 0.04).astype(np.uint8)
    syn = ((Hd.astype(np.int64) @ e.T.astype(np.int64)) % 2).T.astype(np.uint8)
    syn[40:, :] = rng.integers(0, 2, size=(25, 27))   # arbitrary syndromes; some set the empty check's entry
    assert syn[:, 0].any() and not syn[:40, 0].any()
    return sp.csc_matrix(Hd), prior, syn


def test_irregular_graph_every_record_form_and_every_bit_pinned(ldpc, gpu):
    H, prior, syn = _irregular()
    want = DecimModel(H, prior, 3, 150).decode(syn)
    err, conv, its, ndec, L = want
    assert int(conv.sum()) == 26 and int(((conv == 1) & (ndec > 0)).sum()) == 25 and int((conv == 0).sum()) == 39
    assert int(ndec.max()) == 150 and int(its.max()) == 453
    pinned = np.abs(L) == np.float32(2e6)
    assert np.array_equal(pinned.sum(axis=1), ndec)
    assert pinned[:, 149].any() and pinned[:, 148].any() and pinned[:, 60:130].any()   # degree 0, degree 1, the per-edge check
    ran = []
    for variant in (1, 2):
        try:
            dec = _decoder(ldpc, H, prior, 3, 150, kernel_variant=variant)
        except ldpc.LdpcError as e:
            assert variant == 1 and e.status == UNSUPPORTED
            continue
        assert dec.kernel == variant
        _both_entries(dec, syn, want, f"tier {variant}")
        ran.append(variant)
        dec.close()
    assert 2 in ran


def test_the_clamp_engages_and_pins_read_twice_the_clip(ldpc, gpu, bb72_case):
    H, syn, prior, _, _ = bb72_case
    model = DecimModel(H, prior, 5, 20, alpha=1.0, clip=8.0)
    want = model.decode(syn[:64])
    D = model.last_D
    free = DecimModel(H, prior, 5, 20, alpha=1.0, clip=1e6).decode(syn[:64])
    assert (want[4].view(np.int32) != free[4].view(np.int32)).any()      # the clamp changes this input's outcome
    assert D.any() and np.array_equal(D.sum(axis=1), want[3]) and (np.abs(want[4][D]) == np.float32(16.0)).all()
    assert (want[4][D] > 0).any() and (want[4][D] < 0).any()             # pins of both signs
    for variant in (1, 2):
        dec = _decoder(ldpc, H, prior, 5, 20, alpha=1.0, clip=8.0, kernel_variant=variant)
        got = _device(dec, syn[:64])
        _same(got, want, f"clip 8, tier {variant}")
        assert (np.abs(got[2][D]) == 16.0).all()                         # a pinned bit reads exactly +-2 clip
        dec.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("cap", [1, 3])
def test_tile_after_tile_in_one_slot_under_a_capped_grid(ldpc, gpu, monkeypatch, bb72_case, cap, variant):
    """All 400 syndromes are 7 tiles on `cap` workgroups, then other columns with the same handle: a tile that follows
    another in the same LDS block or workspace slot must find a cleared D.  The knob is read when the decoder is created;
    setting it selects the experiments build."""
    H, syn, prior, _, short = bb72_case
    monkeypatch.setenv("LDPC_MS_GRID_MAX", str(cap))
    dec = _decoder(ldpc, H, prior, 3, 6, kernel_variant=variant)
    assert dec._L is ldpc._capi.lib(True)
    assert (dec.info().kernel, dec.info().tile_syndromes, dec.info().last_grid) == (variant, 64, 0)
    _same(_device(dec, syn), short, f"tier {variant}, grid {cap}")
    assert dec.info().last_grid == cap < 7
    _same(_device(dec, syn[250:350]), _rows(short, slice(250, 350)), f"tier {variant}, grid {cap}, columns 250:350")
    assert dec.info().last_grid == min(cap, 2)
    _same(_host(dec, syn), short, f"tier {variant}, grid {cap}, host entry")
    assert dec.info().last_grid == cap
    dec.close()


# ---- compositions: model sampler -> model decoder -> model score ---------------------------------------------------

def test_run_trials_equals_model_sampler_model_decoder_model_score(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    dec = ldpc.DecimatedMinSumDecoder(Hx, 0.03, 5, max_decimations=8)
    res = ldpc.run_trials(dec, 1000, per=0.03, batch=256, seed=7, logicals=Lz)
    errors = tm.sample(72, 1000, 0.03, seed=7)
    guesses, conv, _, ndec, _ = DecimModel(Hx, llr_of_probs(np.full(72, 0.03)), 5, 8).decode(tm.syndromes(Hx, errors))
    assert ((conv == 1) & (ndec > 0)).any()
    _, want = tm.score(Hx, Lz, guesses, errors)
    assert res == ldpc.TrialResult(1000, int(want[1]), int(want[2]), int(want[3]), int((conv == 0).sum()))
    assert 0 < res.block_errors < 1000
    dec.close()


def test_bposd_around_a_decimation_decoder(ldpc, gpu):
    import torch

    H, _ = _bb72(ldpc)
    Hd = np.asarray(H.todense()).astype(np.uint8)
    e = np.concatenate([ldpc.codes.random_errors(72, 100, 0.03, seed=4), ldpc.codes.random_errors(72, 100, 0.08, seed=6)])
    syn = ldpc.codes.syndromes_of(H, e)
    prior = llr_of_probs(np.full(72, 0.03))
    merr, mconv, _, mdec, mL = DecimModel(H, prior, 3, 4).decode(syn)   # short rounds, few decimations: unconverged columns for the OSD step
    assert 0 < mconv.sum() < 200 and ((mconv == 0) & (mdec == 4)).any() and ((mconv == 1) & (mdec > 0)).any()
    want = np.stack([osd_model_postprocess(Hd, syn[b], merr[b], mL[b].astype(np.float64), 2) for b in range(200)])
    inner = ldpc.DecimatedMinSumDecoder(H, 0.03, 3, max_decimations=4)
    dec = ldpc.BeliefPropagationOSDDecoder(H, osd_order=2, osd="device", bp_decoder=inner)
    assert dec.bp_decoder is inner
    out, conv, k = dec.batchdecode_device(torch.from_numpy(syn).cuda())
    torch.cuda.synchronize()
    out, conv = out.cpu().numpy(), conv.cpu().numpy()
    assert k == 200 and np.array_equal(conv, mconv)
    assert np.array_equal(out, want), f"{int((out != want).any(axis=1).sum())} columns differ from the model chain"
    assert np.array_equal(ldpc.codes.syndromes_of(H, out), syn)      # every column reproduces its syndrome
    inner.close()
