"""Per-bit sampling rates and detector-error-model trials on the GPU.  Every comparison is against the CPU models
(tests/dem_model.py: the per-bit rule of include/ldpc_mi355x.h restated in numpy; tests/trials_model.py for syndromes
and score; tests/minsum_model.py and tests/relay_model.py for the decoders) and is exact in every element."""
import numpy as np
import pytest
import scipy.sparse as sp

import dem_model as dm
import trials_model as tm
from minsum_model import MinSumModel, llr_of_probs
from relay_model import RelayModel

pytestmark = pytest.mark.gpu

INVALID = 1
RATE_SET = np.array([0.0, 1.0, 2.0 ** -60, 1e-3, 0.25, 1.0 - 2.0 ** -53])
BATCHES = (1, 5, 67)            # 67: ragged against the 4 columns of a workgroup
BIG0 = (1 << 40) + 3


def _np(x):
    return x.cpu().numpy()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} elements differ from the model, first {bad[:6].tolist()}"


def _random_graph(s, n, seed):
    """Three seeded entries in every column."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.choice(s, size=3, replace=False) for _ in range(n)])
    return sp.csc_matrix((np.ones(3 * n, dtype=np.uint8), (rows, np.repeat(np.arange(n), 3))), shape=(s, n))


def _graph(ldpc, n):
    """n = 73: odd, so the columns start at every address mod 16; n = 11: every piece takes the byte path; n = 1000: the
    (10, 9) code, four checks per lane; n = 4099: a workgroup per column, four checks per lane."""
    if n == 1000:
        return ldpc.codes.parity_check_csc(1000, 10, 9)
    return _random_graph({73: 37, 11: 5, 4099: 1030}[n], n, seed=n)


def _rates(n, seed=1):
    """Drawn from RATE_SET, with an always-set and a never-set bit in the first and in the last piece of a column."""
    r = RATE_SET[np.random.default_rng(seed).integers(0, RATE_SET.size, size=n)]
    r[[0, n - 1]] = 1.0
    r[[1, n - 2]] = 0.0
    return r


@pytest.fixture(scope="module")
def wanted():
    """(n, batch, seed, column0) -> the model's errors for _rates(n), computed once."""
    cache = {}

    def get(n, batch, seed, column0):
        key = (n, batch, seed, column0)
        if key not in cache:
            cache[key] = dm.sample(_rates(n), batch, seed, column0)
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", [73, 11, 1000, 4099])
def test_sample_rates_equals_the_model_through_both_entries(ldpc, gpu, wanted, n, variant):
    H = _graph(ldpc, n)
    t = ldpc.Trials(H, kernel_variant=variant)
    assert t.kernel == variant and t.rates is None
    rates = _rates(n)
    assert set(rates.tolist()) == set(RATE_SET.tolist()) or n == 11
    t.set_rates(rates)
    assert np.array_equal(t.rates, rates)
    for B, (seed, c0) in zip(BATCHES, ((0, 0), (0xDEADBEEFCAFE1234, 5), (3, BIG0))):
        want_e = wanted(n, B, seed, c0)
        want_s = tm.syndromes(H, want_e)
        what = f"n {n} tier {variant} batch {B} column0 {c0}"
        e, sy = t.sample_rates(B, seed=seed, column0=c0)
        _same(_np(e), want_e, what + " device errors")
        _same(_np(sy), want_s, what + " device syndromes")
        he, hs = t.sample_rates_host(B, seed=seed, column0=c0)
        _same(he, want_e, what + " host errors")
        _same(hs, want_s, what + " host syndromes")
    t.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_null_syndromes_unaligned_buffers_and_a_split_call(ldpc, gpu, wanted, variant):
    import torch

    n, B = 73, 67
    H = _graph(ldpc, n)
    s = H.shape[0]
    want_e = wanted(n, B, 3, BIG0)
    want_s = tm.syndromes(H, want_e)
    t = ldpc.Trials(H, kernel_variant=variant)
    t.set_rates(_rates(n))
    for off_e, off_s in ((0, 0), (3, 1), (15, 2)):
        buf_e = torch.full((off_e + B * n + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
        buf_s = torch.full((off_s + B * s + 4096,), 0xCD, dtype=torch.uint8, device="cuda")
        e = buf_e[off_e:off_e + B * n].view(B, n)
        sy = buf_s[off_s:off_s + B * s].view(B, s)
        t.sample_rates(B, seed=3, column0=BIG0, out=(e, None))             # errors only
        _same(_np(e), want_e, f"tier {variant} offset {off_e} errors (no syndromes)")
        assert bool((buf_e[:off_e] == 0xAB).all()) and bool((buf_e[off_e + B * n:] == 0xAB).all())
        assert bool((buf_s == 0xCD).all())
        e.fill_(0xAB)
        # one call split in two at an odd column
        t.sample_rates(29, seed=3, column0=BIG0, out=(e[:29], sy[:29]))
        t.sample_rates(B - 29, seed=3, column0=BIG0 + 29, out=(e[29:], sy[29:]))
        _same(_np(e), want_e, f"tier {variant} offset {off_e} errors (split call)")
        _same(_np(sy), want_s, f"tier {variant} offset {off_s} syndromes (split call)")
        assert bool((buf_e[:off_e] == 0xAB).all()) and bool((buf_e[off_e + B * n:] == 0xAB).all())
        assert bool((buf_s[:off_s] == 0xCD).all()) and bool((buf_s[off_s + B * s:] == 0xCD).all())
    e0, s0 = t.sample_rates(0)                                              # batch 0: nothing touched
    assert tuple(e0.shape) == (0, n) and tuple(s0.shape) == (0, s)
    t.close()


@pytest.mark.parametrize("n", [73, 1000, 4099])
def test_equal_rates_equal_the_uniform_sample_on_the_device(ldpc, gpu, n):
    import torch

    H = _graph(ldpc, n)
    t = ldpc.Trials(H)
    for per in (0.0, 0.02, 1.0):
        t.set_rates(np.full(n, per))
        e, sy = t.sample_rates(67, seed=9, column0=BIG0)
        ue, us = t.sample(67, per, seed=9, column0=BIG0)
        assert torch.equal(e, ue) and torch.equal(sy, us), (n, per)
        if per == 0.02:
            _same(_np(e), tm.sample(n, 67, per, 9, BIG0), f"n {n} per {per} against the uniform model")
            assert 0 < int(e.sum()) < e.numel()
    t.close()


def test_a_queued_sample_keeps_the_table_it_was_launched_with(ldpc, gpu):
    """set_rates, a sample on a side stream, set_rates again, a second sample, and only then a host synchronise."""
    import torch

    n, B = 1000, 4096
    H = _graph(ldpc, n)
    first, second = _rates(n, seed=1), _rates(n, seed=2)
    assert not np.array_equal(first, second)
    t = ldpc.Trials(H)
    side = torch.cuda.Stream()
    t.set_rates(first)
    with torch.cuda.stream(side):
        e1, s1 = t.sample_rates(B, seed=4)
    t.set_rates(second)
    assert np.array_equal(t.rates, second)
    with torch.cuda.stream(side):
        e2, s2 = t.sample_rates(B, seed=4)
    side.synchronize()
    want1, want2 = dm.sample(first, B, 4), dm.sample(second, B, 4)
    assert not np.array_equal(want1, want2)
    _same(_np(e1), want1, "errors under the first table")
    _same(_np(s1), tm.syndromes(H, want1), "syndromes under the first table")
    _same(_np(e2), want2, "errors under the second table")
    _same(_np(s2), tm.syndromes(H, want2), "syndromes under the second table")
    t.close()


def test_refusals_leave_the_table_as_it_was(ldpc, gpu, wanted):
    n = 73
    H = _graph(ldpc, n)
    t = ldpc.Trials(H)
    for call in (lambda: t.sample_rates(5), lambda: t.sample_rates_host(5)):   # no table yet
        with pytest.raises(ldpc.LdpcError) as ei:
            call()
        assert ei.value.status == INVALID and "rates" in ei.value.message
    rates = _rates(n)
    t.set_rates(rates)
    for bad, index in ((float("nan"), 5), (-1e-9, 72), (1.0 + 2.0 ** -52, 0)):
        r = rates.copy()
        r[index:min(index + 4, n):3] = bad                                     # (the first offender is the one named)
        with pytest.raises(ldpc.LdpcError) as ei:
            t.set_rates(r)
        assert ei.value.status == INVALID and f"rates[{index}]" in ei.value.message, ei.value.message
        assert t.rates is rates
        _same(_np(t.sample_rates(5, seed=0xDEADBEEFCAFE1234, column0=5)[0]), wanted(n, 5, 0xDEADBEEFCAFE1234, 5), "after a refused table")
    with pytest.raises(ValueError):
        t.set_rates(rates[:-1])
    assert gpu.ldpc_trials_set_rates(t._h, n - 1, rates.ctypes.data) == INVALID and b"n" in gpu.ldpc_last_error()
    _same(t.sample_rates_host(5, seed=0xDEADBEEFCAFE1234, column0=5)[0], wanted(n, 5, 0xDEADBEEFCAFE1234, 5), "after a wrong n")
    t.set_rates(None)                                                          # cleared
    assert t.rates is None
    with pytest.raises(ldpc.LdpcError) as ei:
        t.sample_rates(5)
    assert ei.value.status == INVALID
    _same(_np(t.sample(5, 0.25, seed=1)[0]), tm.sample(n, 5, 0.25, 1), "the uniform sample needs no table")
    t.close()


# ---- detector-error-model runs: model sampler -> model decoder -> model score ----------------------------------------------

TRIALS, BATCH, SEED = 1500, 512, 17
SHORT = [12, 8, 8]


@pytest.fixture(scope="module")
def bb72_dem(ldpc):
    """The phenomenological model of BB-72 H_X at R = 3 (n = 288, s = 108), p = 0.01, q = 0.02, with the model's errors
    and syndromes of the run."""
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    dem = ldpc.phenomenological(Hx, Lz, 3, 0.01, 0.02)
    assert dem.H.shape == (108, 288) and dem.L.shape == (12, 288)
    errors = dm.sample(dem.rates, TRIALS, SEED)
    syn = tm.syndromes(dem.H, errors)
    for a in (errors, syn):
        a.setflags(write=False)
    return dem, errors, syn


def _expect(dem, errors, guesses, conv):
    _, c = tm.score(dem.H, dem.L, guesses, errors)
    return (int(c[0]), int(c[1]), int(c[2]), int(c[3]), int((np.asarray(conv) == 0).sum()))


def _five(res):
    return (res.trials, res.block_errors, res.syndrome_mismatches, res.logical_errors, res.not_converged)


def test_run_dem_trials_of_min_sum_equals_the_models(ldpc, gpu, bb72_dem):
    dem, errors, syn = bb72_dem
    dec = ldpc.MinSumDecoder(dem.H, None, 30, channel_probs=dem.rates)
    res = ldpc.run_dem_trials(dem, dec, TRIALS, batch=BATCH, seed=SEED)
    guesses, conv, _, _ = MinSumModel(dem.H, llr_of_probs(dem.rates), 30).decode(syn)
    want = _expect(dem, errors, guesses, conv)
    print("min-sum:", res)
    assert _five(res) == want
    assert 0 < res.logical_errors <= res.block_errors < TRIALS
    # the same through a handle of the model's own, and whatever the batch
    t = dem.trials()
    _same(_np(t.sample_rates(100, seed=SEED, column0=700)[0]), errors[700:800], "dem.trials()")
    t.close()
    assert _five(ldpc.run_dem_trials(dem, dec, TRIALS, batch=1500, seed=SEED)) == want
    dec.close()


def test_run_dem_trials_of_relay_equals_the_models(ldpc, gpu, bb72_dem):
    dem, errors, syn = bb72_dem
    g = np.empty((3, 288), dtype=np.float32)
    g[0] = 0.125
    g[1:] = np.random.default_rng(5).uniform(-0.24, 0.66, size=(2, 288)).astype(np.float32)
    dec = ldpc.RelayMinSumDecoder(dem.H, None, SHORT[0], channel_probs=dem.rates, legs=3, leg_iters=SHORT[1], gammas=g)
    res = ldpc.run_dem_trials(dem, dec, TRIALS, batch=BATCH, seed=SEED)
    guesses, conv, _, _, _ = RelayModel(dem.H, llr_of_probs(dem.rates), g, SHORT).decode(syn)
    print("relay:", res)
    assert _five(res) == _expect(dem, errors, guesses, conv)
    assert 0 < res.block_errors < TRIALS
    dec.close()


def test_run_dem_trials_of_bp_equals_the_oracle_chain(ldpc, gpu, bb72_dem):
    """BP has one prior for all bits (0.01 here); the trials are drawn at the model's rates all the same."""
    from oracle import BPOracle

    dem, errors, syn = bb72_dem
    dec = ldpc.BeliefPropagationDecoder(dem.H, 0.01, 20)
    res = ldpc.run_dem_trials(dem, dec, TRIALS, batch=BATCH, seed=SEED)
    want = np.zeros(4, dtype=np.int64)
    not_conv = 0
    for c0 in range(0, TRIALS, BATCH):                                        # the same batches, the last one ragged
        g, conv = dec.decode_batch_host(syn[c0:c0 + BATCH])[:2]
        want += tm.score(dem.H, dem.L, g, errors[c0:c0 + BATCH])[1]
        not_conv += int((np.asarray(conv) == 0).sum())
    print("bp:", res)
    assert _five(res) == (TRIALS, int(want[1]), int(want[2]), int(want[3]), not_conv)
    H = sp.csc_matrix(dem.H)
    oerr, oconv, _, _ = BPOracle(csc=(H.indptr, H.indices), shape=H.shape, per=0.01, max_iters=20).batchdecode(syn, want_llr=False)
    assert _five(res) == _expect(dem, errors, oerr, oconv)
    with pytest.raises(ValueError):
        ldpc.run_dem_trials(ldpc.phenomenological(dem.H[:, :72], None, 1, 0.01, 0.02), dec, 10)
    dec.close()
