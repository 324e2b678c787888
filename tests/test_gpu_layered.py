"""The layered min-sum schedule on the GPU against the numpy model of its rule (tests/layered_model.py): equality in every
element -- errors, flags, iteration counts, and the LLRs as bit patterns; the arithmetic has no division and no
transcendental, so there is no tolerance.  The smallest shapes that reach every code path of layered_kernels.hpp: both
tiers, tiles of 64 / 16 / 4 / 2 syndromes, ragged tiles, layers narrower than the thread groups of a workgroup, a layer
of one check, every record form (check degree <= 32, <= 64, per edge), empty and degree-1 nodes, the clamps, slot reuse,
and the compositions with the trials loop, the OSD step and the sliding windows."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import dem_model as dm
import trials_model as tm
import windows_model as wm
from layered_model import LayeredMinSumModel
from minsum_model import MinSumModel, llr_of_probs
from osd_model import osd_model_postprocess
from test_gpu_minsum import _bb72, _device, _irregular, _same
from test_layer_plan_cpu import graphs
from test_gpu_minsum_tiles import batch_of, reuse_preconditions, tiles_of, waterfall_inputs

pytestmark = pytest.mark.gpu


def _frozen(want):
    for x in want:
        x.setflags(write=False)
    return want


@pytest.fixture(scope="module")
def bb72_case(ldpc):
    """BB-72 H_X, uniform prior 0.03; the 200 syndromes of tests/test_gpu_minsum.py (errors sampled at 0.01 / 0.03 / 0.06);
    the layered model at alpha 0.75 and 1."""
    H, _ = _bb72(ldpc)
    e = np.concatenate([ldpc.codes.random_errors(72, 66, 0.01, seed=1), ldpc.codes.random_errors(72, 67, 0.03, seed=2),
                        ldpc.codes.random_errors(72, 67, 0.06, seed=3)])
    syn = ldpc.codes.syndromes_of(H, e)
    prior = llr_of_probs(np.full(72, 0.03))
    ref = {a: _frozen(LayeredMinSumModel(H, prior, 30, alpha=a).decode(syn)) for a in (0.75, 1.0)}
    assert 0 < ref[0.75][1].sum() < 200 and len(set(ref[0.75][2].tolist())) > 3   # converged and not, many iteration counts
    flood = MinSumModel(H, prior, 30).decode(syn)
    assert (flood[3].view(np.int32) != ref[0.75][3].view(np.int32)).any()           # the schedules differ on this input
    return H, syn, ref


@pytest.mark.parametrize("alpha", [0.75, 1.0])
@pytest.mark.parametrize("variant", [0, 2])
def test_bb72_equals_the_model_on_both_tiers_and_both_entries(ldpc, gpu, bb72_case, alpha, variant):
    H, syn, ref = bb72_case
    dec = ldpc.MinSumDecoder(H, 0.03, 30, alpha=alpha, kernel_variant=variant, schedule="layered")
    assert dec.kernel == (2 if variant == 2 else 1) and dec.info().tile_syndromes == 64
    assert dec.layers == 4 and dec.info().layers == 4 and dec.info().schedule == "layered" and gpu.ldpc_minsum_layers(dec._h) == 4
    _same(_device(dec, syn), ref[alpha], "device entry")
    _same(dec.decode_batch_host(syn, want_llr=True), ref[alpha], "host entry")
    assert dec.decode_batch_host(syn)[2] is None
    guess, ok = dec.decode_(syn[5])
    assert np.array_equal(guess, ref[alpha][0][5]) and ok == bool(ref[alpha][1][5])
    assert np.array_equal(dec.scratch.log_probabs, ref[alpha][3][5].astype(np.float64))
    out = np.zeros((72, 200), dtype=np.uint8)
    _, success = dec.batchdecode_(syn.T, out)
    assert np.array_equal(out.T, ref[alpha][0]) and np.array_equal(success, ref[alpha][1].astype(bool))
    dec.close()


@functools.lru_cache(maxsize=None)
def c240_case():
    """(240, 8, 4) with the per-bit priors of tests/test_gpu_minsum.py (three of them negative), batch 130."""
    import ldpcdecoders_jl_amd as ldpc

    H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
    rng = np.random.default_rng(11)
    probs = rng.uniform(1e-4, 0.45, 240)
    probs[[3, 77, 200]] = [0.6, 0.75, 0.9]
    e = (rng.random((130, 240)) < np.minimum(probs, 0.04)[None, :]).astype(np.uint8)
    syn = ldpc.codes.syndromes_of(H, e)
    model = LayeredMinSumModel(H, llr_of_probs(probs), 20)
    assert model.K == 4 and [len(ly) for ly in model.layers] == [30] * 4      # 30 checks a layer: fewer than T / S = 32 at S = 16
    want = _frozen(model.decode(syn))
    assert 0 < want[1].sum() < 130
    return H, probs, syn, want


@pytest.mark.parametrize("variant,S", [(1, 16), (2, 64)])
def test_per_bit_priors_on_240_8_4(ldpc, gpu, variant, S):
    """Batch 130 is ragged on both tiers: eight tiles of 16 and one of 2 on chip -- where a layer has fewer checks than the
    workgroup has thread groups --, two tiles of 64 and one of 2 in the unlimited tier."""
    H, probs, syn, want = c240_case()
    dec = ldpc.MinSumDecoder(H, None, 20, channel_probs=probs, kernel_variant=variant, schedule="layered")
    assert (dec.kernel, dec.info().tile_syndromes, dec.layers) == (variant, S, 4) and (dec.channel_llr < 0).sum() == 3
    _same(_device(dec, syn), want, f"tier {variant}")
    assert dec.info().last_grid == tiles_of(130, S)
    dec.close()


def test_irregular_graph_every_record_form(ldpc, gpu):
    """tests/test_gpu_minsum.py's graph: an empty check (against 0 and 1 entries), degree-1 nodes, an isolated bit, checks
    of degree 33, 64 and 70, a subnormal and a -0 prior; five layers of 3 to 10 checks."""
    H, prior, syn = _irregular()
    model = LayeredMinSumModel(H, prior, 20)
    assert model.K == 5 and model.layer_of[0] == -1 and max(len(ly) for ly in model.layers) < 16
    assert syn[:, 0].any() and not syn[:, 0].all() and prior[7] != 0 and abs(prior[7]) < np.finfo(np.float32).tiny and np.signbit(prior[8])
    want = model.decode(syn)
    assert want[1].any() and not want[1].all() and want[0][:, 149].all()
    for variant in (1, 2):
        dec = ldpc.MinSumDecoder(H, None, 20, channel_llr=prior, kernel_variant=variant, schedule="layered")
        assert dec.kernel == variant and dec.layers == model.K
        _same(_device(dec, syn), want, f"tier {variant}")
        dec.close()


def test_a_check_alone_in_its_layer(ldpc, gpu):
    """tests/test_layer_plan_cpu.py's graph with one row touching every bit (degree 40: two sign words): that row is a
    layer of its own between two layers of the others; arbitrary syndromes, batch 70 (ragged)."""
    H = graphs(ldpc)["one_row_every_bit"][0]
    rng = np.random.default_rng(8)
    prior = llr_of_probs(rng.uniform(0.02, 0.4, 40))
    syn = rng.integers(0, 2, size=(70, 6), dtype=np.uint8)
    syn[:35] = ldpc.codes.syndromes_of(H, (rng.random((35, 40)) < 0.05).astype(np.uint8))
    model = LayeredMinSumModel(H, prior, 15)
    assert [len(ly) for ly in model.layers] == [4, 1, 1] and model.layers[1] == [2]
    want = model.decode(syn)
    assert want[1].any() and not want[1].all()
    for variant in (1, 2):
        dec = ldpc.MinSumDecoder(H, None, 15, channel_llr=prior, kernel_variant=variant, schedule="layered")
        assert dec.kernel == variant and dec.layers == 3
        _same(_device(dec, syn), want, f"tier {variant}")
        dec.close()


def test_clamps_engage(ldpc, gpu):
    H, _ = _bb72(ldpc)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 64, 0.06, seed=9))
    prior = llr_of_probs(np.full(72, 0.06))
    want = LayeredMinSumModel(H, prior, 50, alpha=1.0, clip=8.0).decode(syn)
    free = LayeredMinSumModel(H, prior, 50, alpha=1.0, clip=1e6).decode(syn)
    assert (want[3].view(np.int32) != free[3].view(np.int32)).any()      # the clamp changes this input's outcome
    for variant in (1, 2):
        dec = ldpc.MinSumDecoder(H, 0.06, 50, alpha=1.0, clip=8.0, kernel_variant=variant, schedule="layered")
        _same(_device(dec, syn), want, f"clip 8, tier {variant}")
        dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_max_iters_zero_and_one_and_wide_syndrome_entries(ldpc, gpu, bb72_case, variant):
    H, syn, _ = bb72_case
    prior = llr_of_probs(np.full(72, 0.03))
    dec = ldpc.MinSumDecoder(H, 0.03, 0, kernel_variant=variant, schedule="layered")
    assert dec.layers == 4
    for err, conv, llr, its in (_device(dec, syn[:70]), dec.decode_batch_host(syn[:70], want_llr=True)):
        assert not err.any() and not conv.any() and not its.any() and not llr.view(np.int64).any()
    dec.close()
    dec = ldpc.MinSumDecoder(H, 0.03, 1, kernel_variant=variant, schedule="layered")
    want = LayeredMinSumModel(H, prior, 1).decode(syn[:70])
    assert want[1].any() and not want[1].all()
    _same(_device(dec, syn[:70]), want, "max_iters 1")
    dec.close()
    # an entry that is not 0 counts as 1
    dec = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant, schedule="layered")
    wide = syn[:70].copy()
    wide[wide == 1] = np.where(np.arange((wide == 1).sum()) % 2 == 0, 2, 3)
    wide[0, np.nonzero(syn[0] == 0)[0][:2]] = [255, 128]
    plain = (wide != 0).astype(np.uint8)
    want = LayeredMinSumModel(H, prior, 30).decode(plain)
    _same(_device(dec, wide), want, "entries 2, 3, 128, 255")
    _same(_device(dec, plain), want, "entries 1")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_a_handle_used_three_times_and_optional_outputs(ldpc, gpu, bb72_case, variant):
    H, syn, ref = bb72_case
    dec = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant, schedule="layered")
    for lo, hi in ((150, 151), (0, 129), (199, 200)):
        want = tuple(x[lo:hi] for x in ref[0.75])
        _same(_device(dec, syn[lo:hi]), want, f"columns {lo}:{hi}")
    want = tuple(x[:129] for x in ref[0.75])
    for want_llr in (False, True):
        for want_iters in (False, True):
            _same(_device(dec, syn[:129], want_llr=want_llr, want_iters=want_iters), want, f"llr {want_llr}, iters {want_iters}")
    dec.close()


# ---- small widths ------------------------------------------------------------------------------------------------------

SMALL = {1536: (1, 4, 0), 3072: (1, 2, 0), 768: (2, 64, 2)}     # n -> (tier, S, kernel_variant)
SMALL_ITERS = 6


@functools.lru_cache(maxsize=None)
def small_case(n):
    """The waterfall inputs of tests/test_gpu_minsum_tiles.py ((3,6)-regular, per-bit priors, rows from nearly clean to
    hopeless) at two full tiles and more, and the layered model on them."""
    _, S, _ = SMALL[n]
    H, prior, syn = waterfall_inputs(n, batch_of(S), 0.05)
    model = LayeredMinSumModel(H, prior, SMALL_ITERS)
    want = _frozen(model.decode(syn))
    assert 0 < want[1].sum() < len(syn) and len(set(want[2].tolist())) >= 3, (n, want[1].sum(), sorted(set(want[2].tolist())))
    return H, prior, syn, model.K, want


@pytest.mark.parametrize("n", sorted(SMALL))
def test_small_widths_and_the_forced_unlimited_tier(ldpc, gpu, n):
    tier, S, variant = SMALL[n]
    H, prior, syn, K, want = small_case(n)
    dec = ldpc.MinSumDecoder(H, None, SMALL_ITERS, channel_llr=prior, kernel_variant=variant, schedule="layered")
    assert (dec.kernel, dec.info().tile_syndromes, dec.layers) == (tier, S, K)
    _same(_device(dec, syn), want, f"n {n} tier {tier} S {S}")
    assert dec.info().last_grid == tiles_of(len(syn), S) >= 3
    dec.close()


# ---- slot reuse --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reuse_case():
    """BB-72 H_X, uniform prior 0.06, the 400 syndromes of tests/test_gpu_minsum_tiles.py: seven tiles of 64, the last
    one ragged."""
    import ldpcdecoders_jl_amd as ldpc

    H = sp.csc_matrix(np.asarray(ldpc.codes.bivariate_bicycle_72_12_6()[0], dtype=np.uint8))
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 400, 0.06, seed=3))
    want = _frozen(LayeredMinSumModel(H, llr_of_probs(np.full(72, 0.06)), 30).decode(syn))
    reuse_preconditions(want[1], None, 400, 64, (1, 3))
    return H, syn, want


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_tile_after_tile_in_one_slot_under_a_capped_grid(ldpc, gpu, monkeypatch, variant, cap):
    """One handle of the experiments build, three calls in a row: 1 tile, then all 7 on `cap` workgroups, then 2 tiles of
    other syndromes -- every state a tile finds is what the tile or the call before left there."""
    H, syn, want = reuse_case()
    monkeypatch.setenv("LDPC_MS_GRID_MAX", str(cap))
    dec = ldpc.MinSumDecoder(H, 0.06, 30, kernel_variant=variant, schedule="layered")
    assert dec._L is ldpc._capi.lib(True) and (dec.kernel, dec.info().tile_syndromes, dec.info().last_grid, dec.layers) == (variant, 64, 0, 4)
    for lo, hi in ((336, 400), (0, 400), (250, 350)):
        _same(_device(dec, syn[lo:hi]), tuple(x[lo:hi] for x in want), f"tier {variant} grid {cap}, columns {lo}:{hi}")
        assert dec.info().last_grid == min(cap, tiles_of(hi - lo, 64))
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_more_tiles_than_resident_workgroups_in_the_product_build(ldpc, gpu, monkeypatch, variant):
    """64 (2 CUs + 1) + 37 syndromes: the 400 known ones repeated with a roll of 13 per repetition; the grid must come out
    smaller than the tile count."""
    import torch

    monkeypatch.delenv("LDPC_MS_GRID_MAX", raising=False)
    assert not ldpc._capi.knobs_in_env()
    H, syn, want = reuse_case()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 * (2 * cus + 1) + 37
    b = np.arange(B)
    idx = (b + 13 * (b // 400)) % 400
    dec = ldpc.MinSumDecoder(H, 0.06, 30, kernel_variant=variant, schedule="layered")
    assert dec._L is ldpc._capi.lib(False) and (dec.kernel, dec.info().tile_syndromes) == (variant, 64)
    got = _device(dec, syn[idx])
    assert 0 < dec.info().last_grid < tiles_of(B, 64), (dec.info(), B)
    _same(got, tuple(x[idx] for x in want), f"tier {variant}, batch {B}")
    dec.close()


# ---- against the library itself ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
def test_schedule_flooding_is_the_decoder_without_the_keyword(ldpc, gpu, bb72_case, variant):
    H, syn, _ = bb72_case
    plain = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant)
    named = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant, schedule="flooding")
    assert plain.schedule == named.schedule == "flooding" and plain.layers == named.layers == 0 and named.info().layers == 0
    a, b = _device(plain, syn), _device(named, syn)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    _same(b, MinSumModel(H, llr_of_probs(np.full(72, 0.03)), 30).decode(syn), "flooding")
    plain.close(); named.close()


# ---- compositions --------------------------------------------------------------------------------------------------

def test_run_trials_equals_model_sampler_model_decoder_model_score(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    dec = ldpc.MinSumDecoder(Hx, 0.03, 30, schedule="layered")
    res = ldpc.run_trials(dec, 1000, per=0.03, batch=256, seed=7, logicals=Lz)
    errors = tm.sample(72, 1000, 0.03, seed=7)
    guesses, conv, _, _ = LayeredMinSumModel(Hx, llr_of_probs(np.full(72, 0.03)), 30).decode(tm.syndromes(Hx, errors))
    _, want = tm.score(Hx, Lz, guesses, errors)
    assert res == ldpc.TrialResult(1000, int(want[1]), int(want[2]), int(want[3]), int((conv == 0).sum()))
    assert 0 < res.block_errors < 1000
    dec.close()


def test_bposd_around_a_layered_decoder(ldpc, gpu):
    import torch

    H, _ = _bb72(ldpc)
    Hd = np.asarray(H.todense()).astype(np.uint8)
    e = np.concatenate([ldpc.codes.random_errors(72, 100, 0.03, seed=4), ldpc.codes.random_errors(72, 100, 0.08, seed=6)])
    syn = ldpc.codes.syndromes_of(H, e)
    merr, mconv, _, mL = LayeredMinSumModel(H, llr_of_probs(np.full(72, 0.03)), 30).decode(syn)
    assert 0 < mconv.sum() < 200
    want = np.stack([osd_model_postprocess(Hd, syn[b], merr[b], mL[b].astype(np.float64), 2) for b in range(200)])
    ms = ldpc.MinSumDecoder(H, 0.03, 30, schedule="layered")
    dec = ldpc.BeliefPropagationOSDDecoder(H, osd_order=2, osd="device", bp_decoder=ms)
    assert dec.bp_decoder is ms
    out, conv, k = dec.batchdecode_device(torch.from_numpy(syn).cuda())
    torch.cuda.synchronize()
    out, conv = out.cpu().numpy(), conv.cpu().numpy()
    assert k == 200 and np.array_equal(conv, mconv)
    assert np.array_equal(out, want), f"{int((out != want).any(axis=1).sum())} columns differ from the model chain"
    assert np.array_equal(ldpc.codes.syndromes_of(H, out), syn)      # every column reproduces its syndrome
    ms.close()


def test_sliding_windows_of_layered_decoders_equal_the_model_chain(ldpc, gpu):
    """The BB-72 phenomenological fixture of tests/test_gpu_windows.py (R = 5, W = 3, C = 1, 200 syndromes of seed 7):
    tests/windows_model.py around the layered model against SlidingWindowDecoder around layered decoders."""
    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    logicals = ldpc.codes.css_logicals(HX, HZ)[1]
    dem = ldpc.phenomenological(HX, logicals, 5, 0.01, 0.02)
    syn = tm.syndromes(dem.H, dm.sample(dem.rates, 200, 7, 0))
    layers = ldpc.phenomenological_layers(HX, 5)
    windows, uncovered = wm.plan(dem.H, layers, 3, 1)

    def model_of(H, rates):
        model = LayeredMinSumModel(H, llr_of_probs(rates), 30)
        return lambda s: model.decode(s)[:2]
    want = wm.chain(dem.H, dem.rates, windows, uncovered, model_of, syn)[:3]
    assert 0 < int(want[1].sum()) < 200
    dec = ldpc.SlidingWindowDecoder(dem, layers, 3, 1, lambda m: ldpc.MinSumDecoder(m.H, None, 30, channel_probs=m.rates, schedule="layered"))
    assert all(d.schedule == "layered" and d.layers > 0 for d in dec.decoders)
    guess, conv, residual = dec.decode_batch_host(syn)
    for got, w, what in ((guess, want[0], "errors"), (conv, want[1], "flags"), (residual, want[2], "residual")):
        assert np.array_equal(np.asarray(got), np.asarray(w)), what
    dec.close()
