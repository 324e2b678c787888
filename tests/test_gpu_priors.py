"""Min-sum with per-syndrome priors on the GPU against the numpy models of tests/priors_model.py: equality in every element
-- errors, flags, iteration counts, and the LLRs as bit patterns after exact widening; there is no tolerance.  Both
schedules, both tiers, both sources of the priors (floats, given bits), ragged tiles and more than one tile, the second
plan of a flooding handle (another S, another tier than the plain entries of the same handle), slot reuse under a capped
grid, columns with a non-finite prior, the host forms, the refusals that need a handle, and the correlated CSS trials
loop against the model pipeline."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import priors_model as pm
from layered_model import LayeredMinSumModel
from minsum_model import MinSumModel, llr_of_probs
from test_gpu_minsum import _bb72, _device, _same

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5
SCHEDULES = ["flooding", "layered"]
F = np.float32


def _entry(dec, syn, extra, kind, want_llr=True, want_iters=True):
    """The device form of the floats (`kind` "priors") or the given-bits (`kind` "given") entry, as test_gpu_minsum._device."""
    import torch

    B = syn.shape[0]
    d_syn = torch.from_numpy(np.array(syn, dtype=np.uint8)).cuda()                # (copies: the shared inputs are read-only)
    d_extra = torch.from_numpy(np.array(extra, dtype=np.float32 if kind == "priors" else np.uint8)).cuda()
    err = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    (dec.decode_batch_priors_device if kind == "priors" else dec.decode_batch_given_device)(d_syn, d_extra, err, conv, llr, its)
    torch.cuda.synchronize()
    return (err.cpu().numpy(), conv.cpu().numpy(), llr.cpu().numpy() if want_llr else None,
            its.cpu().numpy() if want_iters else None)


def _rows(want, sel):
    return tuple(x[sel] for x in want)


def _frozen(want):
    for x in want:
        x.setflags(write=False)
    return want


def _shared_model(schedule):
    return LayeredMinSumModel if schedule == "layered" else MinSumModel


# ---- BB-72: a conditional-style mix of two tables, odd values in a few places -------------------------------------------------

@functools.lru_cache(maxsize=None)
def bb72_inputs():
    """130 syndromes of errors at 0.06; per row the priors where(random bits, b_j, a_j) of two per-bit tables, with negative
    entries, +0, -0 and a subnormal in a few places; `given` holds the bits as 0 .. 3 (the low bit is the bit)."""
    import ldpcdecoders_jl_amd as ldpc

    H, _ = _bb72(ldpc)
    rng = np.random.default_rng(17)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 130, 0.06, seed=5))
    a, b = llr_of_probs(rng.uniform(0.02, 0.2, 72)), llr_of_probs(rng.uniform(0.3, 0.7, 72))
    a[[4, 40]] = [-1.5, -0.25]
    a[9], a[10], b[11] = F(0.0), F(-0.0), F(1e-41)
    bits = rng.integers(0, 2, size=(130, 72), dtype=np.uint8)
    given = (bits | (rng.integers(0, 2, size=(130, 72), dtype=np.uint8) << 1)).astype(np.uint8)
    assert set(np.unique(given)) == {0, 1, 2, 3} and (b < 0).any() and np.signbit(a[10]) and 0 < b[11] < np.finfo(F).tiny
    pri = pm.select_priors(given, a, b)
    assert np.array_equal(pri.view(np.int32), np.where(bits == 1, b, a).view(np.int32))
    for x in (syn, a, b, given, pri):
        x.setflags(write=False)
    return H, syn, a, b, given, pri


@functools.lru_cache(maxsize=None)
def bb72_want(schedule, max_iters):
    H, syn, _, _, _, pri = bb72_inputs()
    want = _frozen(pm.model_of(schedule, H, max_iters).decode(syn, pri))
    if max_iters == 30:
        assert 0 < want[1].sum() < 130 and len(set(want[2].tolist())) > 3
    if max_iters == 2 and schedule == "flooding":   # the second bit sweep adds the column's OWN prior: the shared one gives another L
        other = MinSumModel(H, pri[0], 2).decode(syn)
        assert (other[3][1:].view(np.int32) != want[3][1:].view(np.int32)).any()
    return want


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_bb72_floats_and_given_entries_equal_the_model(ldpc, gpu, schedule, variant):
    """Batches 1, 63, 65 and 130 (ragged tiles, more than one tile), max_iters 1, 2 and 30; the given entry is the floats
    entry fed where(given & 1, llr_if1, llr_if0) in every bit, with given values 0 .. 3."""
    H, syn, a, b, given, pri = bb72_inputs()
    for max_iters in (1, 2, 30):
        want = bb72_want(schedule, max_iters)
        dec = ldpc.MinSumDecoder(H, 0.03, max_iters, kernel_variant=variant, schedule=schedule)
        info = dec.info()
        assert (info.kernel, info.tile_syndromes, info.priors_kernel, info.priors_tile_syndromes) == (variant, 64, variant, 64)
        assert gpu.ldpc_minsum_priors_kernel(dec._h) == variant and gpu.ldpc_minsum_priors_tile_syndromes(dec._h) == 64
        dec.set_conditional_priors(a, b)
        assert np.array_equal(dec.conditional_llr[0].view(np.int32), a.view(np.int32))
        for B in (1, 63, 65, 130):
            what = f"{schedule} tier {variant} max_iters {max_iters} batch {B}"
            _same(_entry(dec, syn[:B], pri[:B], "priors"), _rows(want, slice(0, B)), what + ", floats")
            assert dec.info().last_grid == (B + 63) // 64
            _same(_entry(dec, syn[:B], given[:B], "given"), _rows(want, slice(0, B)), what + ", given")
        dec.close()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_a_second_set_of_tables_takes_effect_on_the_next_call(ldpc, gpu, schedule):
    H, syn, a, b, given, pri = bb72_inputs()
    dec = ldpc.MinSumDecoder(H, 0.03, 30, schedule=schedule)
    dec.set_conditional_priors(a, b)
    _same(_entry(dec, syn[:70], given[:70], "given"), _rows(bb72_want(schedule, 30), slice(0, 70)), "first tables")
    dec.set_conditional_priors(probs_if0=np.full(72, 0.02), probs_if1=0.5)         # probabilities, a scalar for every bit
    t0, t1 = llr_of_probs(np.full(72, 0.02)), llr_of_probs(np.full(72, 0.5))
    assert np.array_equal(dec.conditional_llr[0].view(np.int32), t0.view(np.int32)) and not dec.conditional_llr[1].any()
    want = pm.model_of(schedule, H, 30).decode(syn[:70], pm.select_priors(given[:70], t0, t1))
    assert (want[3].view(np.int32) != bb72_want(schedule, 30)[3][:70].view(np.int32)).any()
    _same(_entry(dec, syn[:70], given[:70], "given"), want, "second tables")
    _same(dec.decode_batch_given_host(syn[:70], given[:70], want_llr=True), want, "second tables, host form")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_rows_equal_to_channel_llr_give_the_plain_entry(ldpc, gpu, schedule, variant):
    H, syn, a, _, _, _ = bb72_inputs()
    dec = ldpc.MinSumDecoder(H, None, 30, channel_llr=a, kernel_variant=variant, schedule=schedule)
    plain = _device(dec, syn.copy())
    for x, y in zip(_entry(dec, syn, np.tile(dec.channel_llr, (130, 1)), "priors"), plain):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{schedule} tier {variant}: floats entry differs from the plain entry"
    dec.set_conditional_priors(a, a)
    for x, y in zip(_entry(dec, syn, np.arange(130 * 72, dtype=np.uint8).reshape(130, 72), "given"), plain):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{schedule} tier {variant}: given entry differs from the plain entry"
    _same(plain, _shared_model(schedule)(H, a, 30).decode(syn), "plain entry")
    dec.close()


def test_host_forms_equal_the_device_forms(ldpc, gpu):
    H, syn, a, b, given, pri = bb72_inputs()
    for schedule in SCHEDULES:
        want = bb72_want(schedule, 30)
        dec = ldpc.MinSumDecoder(H, 0.03, 30, schedule=schedule)
        dec.set_conditional_priors(a, b)
        _same(dec.decode_batch_priors_host(syn, pri, want_llr=True), want, schedule + " floats, host")
        _same(dec.decode_batch_given_host(syn, given, want_llr=True), want, schedule + " given, host")
        assert dec.decode_batch_priors_host(syn[:3], pri[:3])[2] is None
        for want_llr in (False, True):
            for want_iters in (False, True):
                _same(_entry(dec, syn[:65], pri[:65], "priors", want_llr, want_iters), _rows(want, slice(0, 65)), "optional outputs")
        with pytest.raises(ValueError):
            dec.decode_batch_priors_host(syn, pri[:, :71])
        dec.close()
    # max_iters = 0 and batch = 0
    dec = ldpc.MinSumDecoder(H, 0.03, 0)
    dec.set_conditional_priors(a, b)
    for got in (_entry(dec, syn[:70], pri[:70], "priors"), _entry(dec, syn[:70], given[:70], "given"),
                dec.decode_batch_priors_host(syn[:70], pri[:70], want_llr=True)):
        err, conv, llr, its = got
        assert not err.any() and not conv.any() and not its.any() and not llr.view(np.int64).any()
    assert gpu.ldpc_minsum_decode_batch_priors(dec._h, 0, None, None, None, None, None, None) == 0
    assert gpu.ldpc_minsum_decode_batch_given_device(dec._h, 0, None, None, None, None, None, None, None) == 0
    dec.close()


# ---- the second plan ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def regular_8_4(n, B, max_iters, seed):
    import ldpcdecoders_jl_amd as ldpc

    H = sp.csc_matrix(ldpc.parity_check_matrix(n, 8, 4))
    assert H.shape == (n // 2, n) and set(np.diff(sp.csr_matrix(H).indptr)) == {8}
    rng = np.random.default_rng(seed)
    syn = ldpc.codes.syndromes_of(H, (rng.random((B, n)) < 0.03).astype(np.uint8))
    shared = llr_of_probs(rng.uniform(0.01, 0.08, n))
    pri = llr_of_probs(rng.uniform(0.01, 0.2, (B, n)))
    want_plain = _frozen(MinSumModel(H, shared, max_iters).decode(syn))
    want_pri = _frozen(pm.PriorsMinSumModel(H, max_iters).decode(syn, pri))
    return H, syn, shared, pri, want_plain, want_pri


def test_n96_plain_at_64_and_priors_at_32_syndromes_interleaved_on_one_handle(ldpc, gpu):
    """12.5 n = 1200 bytes a syndrome fit 79 KiB 64 times, 16.5 n = 1584 bytes only 32 times.  Batch 150: three tiles of 64
    (the last ragged) for the plain entry, five of 32 for the priors entry."""
    H, syn, shared, pri, want_plain, want_pri = regular_8_4(96, 150, 12, 1)
    assert 0 < want_pri[1].sum() < 150
    dec = ldpc.MinSumDecoder(H, None, 12, channel_llr=shared)
    info = dec.info()
    assert (info.kernel, info.tile_syndromes, info.priors_kernel, info.priors_tile_syndromes) == (1, 64, 1, 32)
    given = np.random.default_rng(2).integers(0, 4, size=(150, 96), dtype=np.uint8)
    t0, t1 = pri[0].copy(), pri[1].copy()
    dec.set_conditional_priors(t0, t1)
    want_given = pm.PriorsMinSumModel(H, 12).decode(syn, pm.select_priors(given, t0, t1))
    for k in range(2):
        _same(_device(dec, syn), want_plain, f"plain, round {k}")
        assert dec.info().last_grid == 3
        _same(_entry(dec, syn, pri, "priors"), want_pri, f"priors, round {k}")
        assert dec.info().last_grid == 5
        _same(_entry(dec, syn, given, "given"), want_given, f"given, round {k}")
    dec.close()


def test_n10240_plain_on_chip_and_priors_in_the_unlimited_tier_of_one_handle(ldpc, gpu):
    """128,000 bytes for one syndrome fit 159 KiB, 168,960 with the priors do not: the priors entry runs in the unlimited
    tier (S = 64) while the plain entry of the same handle stays on chip (S = 1).  Forced on-chip, the handle still
    decodes plainly and refuses the priors entries."""
    H, syn, shared, pri, want_plain, want_pri = regular_8_4(10240, 3, 2, 3)
    dec = ldpc.MinSumDecoder(H, None, 2, channel_llr=shared)
    info = dec.info()
    assert (info.kernel, info.tile_syndromes, info.priors_kernel, info.priors_tile_syndromes) == (1, 1, 2, 64)
    _same(_entry(dec, syn, pri, "priors"), want_pri, "priors, unlimited tier")
    assert dec.info().last_grid == 1
    _same(_device(dec, syn), want_plain, "plain, on chip")
    assert dec.info().last_grid == 3
    _same(_entry(dec, syn, pri, "priors"), want_pri, "priors again")
    dec.close()
    dec = ldpc.MinSumDecoder(H, None, 2, channel_llr=shared, kernel_variant=1)
    info = dec.info()
    assert (info.kernel, info.tile_syndromes, info.priors_kernel, info.priors_tile_syndromes) == (1, 1, 0, 0)
    with pytest.raises(ldpc.LdpcError) as e:
        _entry(dec, syn, pri, "priors")
    assert e.value.status == UNSUPPORTED
    dec.set_conditional_priors(shared, shared)
    with pytest.raises(ldpc.LdpcError) as e:
        _entry(dec, syn, np.zeros((3, 10240), dtype=np.uint8), "given")
    assert e.value.status == UNSUPPORTED
    _same(_device(dec, syn), want_plain, "plain, forced on chip")
    dec.close()


# ---- slot reuse -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reuse_want(schedule):
    """Batch 200 = four tiles of 64, the last ragged; every tile has priors of its own (another rate per row)."""
    import ldpcdecoders_jl_amd as ldpc

    H, _ = _bb72(ldpc)
    rng = np.random.default_rng(23)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 200, 0.06, seed=4))
    t0 = llr_of_probs(rng.uniform(0.02, 0.1, 72))
    t1 = llr_of_probs(rng.uniform(0.2, 0.6, 72))
    given = rng.integers(0, 4, size=(200, 72), dtype=np.uint8)
    given[64:128] |= 1                  # tile 1 takes llr_if1 everywhere, tile 2 llr_if0: a P left over from the tile before shows
    given[128:192] &= 2
    pri = pm.select_priors(given, t0, t1)
    want = _frozen(pm.model_of(schedule, H, 30).decode(syn, pri))
    stale = pm.model_of(schedule, H, 30).decode(syn[128:192], pri[64:128])
    assert (stale[3].view(np.int32) != want[3][128:192].view(np.int32)).any() and 0 < want[1].sum() < 200
    return H, syn, t0, t1, given, pri, want


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_tile_after_tile_in_one_slot_under_a_capped_grid(ldpc, gpu, monkeypatch, schedule, variant):
    H, syn, t0, t1, given, pri, want = reuse_want(schedule)
    monkeypatch.setenv("LDPC_MS_GRID_MAX", "1")
    dec = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant, schedule=schedule)
    assert dec._L is ldpc._capi.lib(True) and (dec.info().priors_kernel, dec.info().priors_tile_syndromes) == (variant, 64)
    dec.set_conditional_priors(t0, t1)
    for kind, extra in (("priors", pri), ("given", given)):
        _same(_entry(dec, syn, extra, kind), want, f"{schedule} tier {variant} {kind}, four tiles on one workgroup")
        assert dec.info().last_grid == 1
        _same(_entry(dec, syn[100:170], extra[100:170], kind), _rows(want, slice(100, 170)), f"{schedule} tier {variant} {kind}, another call")
    dec.close()


# ---- non-finite priors --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_a_column_with_a_non_finite_prior_is_not_decoded(ldpc, gpu, schedule, variant):
    H, syn, a, b, given, pri = bb72_inputs()
    bad = pri.copy()
    bad[5, 70], bad[64, 3] = np.nan, np.inf          # one entry each, in the first tile and in the next one
    want = pm.model_of(schedule, H, 30).decode(syn, bad)
    clean = bb72_want(schedule, 30)
    keep = np.ones(130, dtype=bool)
    keep[[5, 64]] = False
    assert all(np.array_equal(x[keep].view(np.uint8), y[keep].view(np.uint8)) for x, y in zip(want, clean))
    dec = ldpc.MinSumDecoder(H, 0.03, 30, kernel_variant=variant, schedule=schedule)
    got = _entry(dec, syn, bad, "priors")
    for c in (5, 64):
        assert not got[0][c].any() and got[1][c] == 0 and got[3][c] == 0 and not got[2][c].view(np.int64).any(), c
    _same(got, want, f"{schedule} tier {variant}")
    bad[129, 0] = -np.inf                            # ... and in the ragged last tile; -inf and a NaN with a payload
    bad[5, 70] = np.array([0xffc00001], dtype=np.uint32).view(F)[0]
    _same(_entry(dec, syn, bad, "priors"), pm.model_of(schedule, H, 30).decode(syn, bad), "second call")
    _same(_entry(dec, syn, pri, "priors"), clean, "the clean priors afterwards")
    dec.close()


# ---- the refusals that need a handle ------------------------------------------------------------------------------------------

def test_refusals_on_a_live_handle(ldpc, gpu):
    import torch

    H, syn, a, b, given, pri = bb72_inputs()
    dec = ldpc.MinSumDecoder(H, 0.03, 30)
    L, h = dec._L, dec._h
    d = {k: torch.from_numpy(np.array(v[:4])).cuda() for k, v in (("syn", syn), ("pri", pri), ("given", given))}
    err, conv = torch.zeros((4, 72), dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731
    # the given entries before any tables
    assert L.ldpc_minsum_decode_batch_given_device(h, 4, p(d["syn"]), p(d["given"]), p(err), p(conv), None, None, None) == INVALID
    assert "ldpc_minsum_set_conditional_priors" in L.ldpc_last_error().decode()
    out = np.zeros((4, 72), dtype=np.uint8)
    assert L.ldpc_minsum_decode_batch_given(h, 4, syn.ctypes.data, given.ctypes.data, out.ctypes.data, out.ctypes.data, None, None) == INVALID
    # non-finite or NULL tables
    for t0, t1 in ((np.where(np.arange(72) == 3, np.nan, a), b), (a, np.where(np.arange(72) == 71, np.inf, b))):
        with pytest.raises(ldpc.LdpcError) as e:
            dec.set_conditional_priors(t0.astype(F), t1.astype(F))
        assert e.value.status == INVALID and "not finite" in e.value.message
    assert dec.conditional_llr is None
    assert L.ldpc_minsum_set_conditional_priors(h, None, b.ctypes.data) == INVALID
    assert L.ldpc_minsum_set_conditional_priors(h, a.ctypes.data, None) == INVALID
    with pytest.raises(TypeError):
        dec.set_conditional_priors(a)
    with pytest.raises(TypeError):
        dec.set_conditional_priors(a, b, probs_if0=np.full(72, 0.1))
    with pytest.raises(ValueError):
        dec.set_conditional_priors(probs_if0=np.full(72, 0.1), probs_if1=1.0)
    with pytest.raises(ValueError):
        dec.set_conditional_priors(a[:71], b)
    dec.set_conditional_priors(a, b)
    # NULL required pointers, a negative batch
    for args in ((None, p(d["pri"]), p(err), p(conv)), (p(d["syn"]), None, p(err), p(conv)), (p(d["syn"]), p(d["pri"]), None, p(conv)),
                 (p(d["syn"]), p(d["pri"]), p(err), None)):
        assert L.ldpc_minsum_decode_batch_priors_device(h, 4, *args, None, None, None) == INVALID, args
        assert "NULL" in L.ldpc_last_error().decode()
    assert L.ldpc_minsum_decode_batch_given_device(h, 4, p(d["syn"]), None, p(err), p(conv), None, None, None) == INVALID
    assert L.ldpc_minsum_decode_batch_priors(h, 4, syn.ctypes.data, None, out.ctypes.data, out.ctypes.data, None, None) == INVALID
    assert L.ldpc_minsum_decode_batch_given(h, 4, syn.ctypes.data, None, out.ctypes.data, out.ctypes.data, None, None) == INVALID
    assert L.ldpc_minsum_decode_batch_priors_device(h, -1, p(d["syn"]), p(d["pri"]), p(err), p(conv), None, None, None) == INVALID
    assert dec.info().last_grid == 0                                    # nothing was launched
    torch.cuda.synchronize()
    assert not err.any() and not conv.any()
    dec.close()


# ---- the correlated trials loop -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", SCHEDULES)
def test_correlated_css_trials_equal_the_model_pipeline(ldpc, gpu, schedule):
    """sample -> model decode on Hz -> select -> model decode on Hx with the selected priors -> score."""
    Hx, Hz = _bb72(ldpc)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    p, marginal = 0.06, 2 * 0.06 / 3
    dec_hx = ldpc.MinSumDecoder(Hx, marginal, 30, schedule=schedule)
    dec_hz = ldpc.MinSumDecoder(Hz, marginal, 30, schedule=schedule)
    res = ldpc.run_css_trials(dec_hx, dec_hz, 1000, p, batch=256, seed=3, correlated=True)
    p_if0, p_if1 = pm.conditional_probs(p)
    t0, t1 = llr_of_probs(np.full(72, p_if0)), llr_of_probs(np.full(72, p_if1))
    assert np.array_equal(dec_hx.conditional_llr[0].view(np.int32), t0.view(np.int32))
    assert np.array_equal(dec_hx.conditional_llr[1].view(np.int32), t1.view(np.int32)) and dec_hz.conditional_llr is None
    ex, ez = cm.sample(72, 1000, p, seed=3)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    gx, cz, _, _ = _shared_model(schedule)(Hz, llr_of_probs(np.full(72, marginal)), 30).decode(sz)
    gz, cx, _, _ = pm.model_of(schedule, Hx, 30).decode(sx, pm.select_priors(gx, t0, t1))
    _, counts = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    want = ldpc.CSSTrialResult(*(int(c) for c in counts), int((cx == 0).sum()), int((cz == 0).sum()))
    assert res == want, (res, want)
    # correlated=False is the call without the keyword, and differs from the correlated run on the Z side only
    plain = ldpc.run_css_trials(dec_hx, dec_hz, 1000, p, batch=256, seed=3)
    named = ldpc.run_css_trials(dec_hx, dec_hz, 1000, p, batch=256, seed=3, correlated=False)
    gz0, cx0, _, _ = _shared_model(schedule)(Hx, llr_of_probs(np.full(72, marginal)), 30).decode(sx)
    _, counts0 = cm.score(Hx, Hz, Lx, Lz, gx, gz0, ex, ez)
    assert plain == named == ldpc.CSSTrialResult(*(int(c) for c in counts0), int((cx0 == 0).sum()), int((cz == 0).sum()))
    assert res.logical_x_errors == plain.logical_x_errors and res.logical_z_errors < plain.logical_z_errors
    # the result does not depend on the batch
    assert ldpc.run_css_trials(dec_hx, dec_hz, 1000, p, batch=1000, seed=3, correlated=True) == res
    dec_hx.close()
    dec_hz.close()


def test_correlated_needs_a_min_sum_decoder_on_hx(ldpc, gpu):
    Hx, Hz = _bb72(ldpc)
    ms = ldpc.MinSumDecoder(Hz, 0.04, 30)
    bp = ldpc.BeliefPropagationDecoder(Hx, 0.04, 30)
    osd = ldpc.BeliefPropagationOSDDecoder(Hx, osd_order=0, bp_decoder=ldpc.MinSumDecoder(Hx, 0.04, 30))
    for bad in (bp, osd):
        with pytest.raises(TypeError, match="MinSumDecoder"):
            ldpc.run_css_trials(bad, ms, 100, 0.06, batch=64, correlated=True)
    # ... while decoder_hz may be any decoder the loop takes: BP on Hz, min-sum on Hx
    bz = ldpc.BeliefPropagationDecoder(Hz, 0.04, 30)
    mx = ldpc.MinSumDecoder(Hx, 0.04, 30, schedule="layered")
    res = ldpc.run_css_trials(mx, bz, 300, 0.06, batch=128, seed=1, correlated=True)
    assert res.trials == 300 and 0 < res.block_errors < 300
    for d in (ms, bp, mx, bz):
        d.close()
