"""Sliding-window decoding on the GPU: the window step kernel alone and `SlidingWindowDecoder` around min-sum, relay, BP
and BP+OSD.  Every comparison is against the CPU models (tests/windows_model.py: plan, gather, commit and the chain,
written from include/ldpc_mi355x.h; minsum_model.py, relay_model.py, osd_model.py and the BP oracle for the decoders) and
is exact in every element.  tests/test_windows_cpu.py asserts on the model that the BB-72 fixture below is not vacuous:
unconverged columns in every window, commits that flip later detectors, columns with a non-zero final residual, and a
guess that differs from the one-shot decode."""
import numpy as np
import pytest
import scipy.sparse as sp

import dem_model as dm
import trials_model as tm
import windows_model as wm
from minsum_model import MinSumModel, llr_of_probs
from osd_model import osd_model_postprocess
from relay_model import RelayModel

pytestmark = pytest.mark.gpu

INVALID = 1
POISON = 0xA5
BATCHES = (1, 5, 67)            # 67: ragged against the 4 columns of a workgroup


def _np(x):
    return x.cpu().numpy()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} elements differ from the model, first {bad[:6].tolist()}"


# ---- the step kernel alone ---------------------------------------------------------------------------------------------

def _random_step(D, N, K, seed):
    """A random H (three entries a column where D allows) and K windows that no layer rule made: every mechanism is owned by
    at most one window (or by none), mech_k holds the owned ones and strangers, det_k is a random NON-contiguous subset.
    Window 0 owns 70 mechanisms that all touch detector D - 1; window K - 2 commits nothing; no column touches detector 0."""
    rng = np.random.default_rng(seed)
    deg = min(3, D)
    rows = np.concatenate([1 + rng.choice(D - 1, size=deg, replace=False) for _ in range(N)])   # detector 0: in no column
    H = sp.lil_matrix((D, N), dtype=np.uint8)
    H[rows, np.repeat(np.arange(N), deg)] = 1
    owner = rng.integers(-1, K, size=N)
    owner[owner == K - 2] = -1
    heavy = np.arange(N)[::max(N // 70, 1)][:70] if N >= 70 else np.arange(0)
    if heavy.size:
        owner[heavy] = 0
        H[D - 1, heavy] = 1
    H = sp.csc_matrix(H)
    H.sort_indices()
    windows = []
    for k in range(K):
        own = np.flatnonzero(owner == k)
        strangers = np.flatnonzero(rng.random(N) < 0.3)
        mech = np.union1d(own, strangers).astype(np.int64)
        chosen = rng.random(D) < 0.6
        chosen[:3] = [True, False, True]
        det = np.flatnonzero(chosen).astype(np.int64)
        if D == 1030 and k == 0:
            mech = np.arange(N, dtype=np.int64)                    # a guess column of more than 4096 bytes: a workgroup per column
        windows.append(dict(det=det, mech=mech, commit=np.searchsorted(mech, own).astype(np.int64)))
    return H, windows


def _offset(x, torch):
    """x (numpy uint8) one byte into a larger poisoned allocation: (view, whole buffer)."""
    buf = torch.full((1 + x.size + 77,), POISON, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + x.size].view(*x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return view, buf


def _untouched(buf, size):
    return bool((buf[:1] == POISON).all()) and bool((buf[1 + size:] == POISON).all())


@pytest.mark.parametrize("D,N,K", [(37, 300, 4), (5, 11, 3), (1030, 4500, 3)])
def test_step_kernel_equals_the_model(ldpc, gpu, D, N, K):
    import torch

    H, windows = _random_step(D, N, K, seed=D)
    cols = wm._columns(H)
    if N >= 70:
        in_row = [c for c in windows[0]["commit"] if D - 1 in cols[int(windows[0]["mech"][c])]]
        assert len(in_row) >= 70                                   # a detector with 70 committed entries in its row
    assert windows[K - 2]["commit"].size == 0                      # a window that commits nothing
    for k in range(K - 1):                                         # a detector owned through det_{k+1} alone
        touched = {d for c in windows[k]["commit"] for d in cols[int(windows[k]["mech"][c])]}
        assert set(windows[k + 1]["det"].tolist()) - touched or D == 5
        assert np.any(np.diff(windows[k]["det"]) > 1)              # non-contiguous
    if D == 1030:
        assert windows[0]["mech"].size > 4096
    step = ldpc.WindowStep(H, [w["det"] for w in windows], [w["mech"] for w in windows], [w["commit"] for w in windows])
    assert len(step) == K
    rng = np.random.default_rng(1000 + D)
    for B in BATCHES:                                              # one handle, batches of different size
        residual = rng.integers(0, 4, size=(B, D), dtype=np.uint8)            # read by the low bit
        residual[:, ::7] = POISON
        guess = np.full((B, N), POISON, dtype=np.uint8)
        conv = rng.integers(0, 3, size=B, dtype=np.uint8)
        d_res, res_buf = _offset(residual, torch)
        d_guess, guess_buf = _offset(guess, torch)
        d_conv, conv_buf = _offset(conv, torch)
        for k, w in enumerate(windows):
            what = f"D {D} batch {B} window {k}"
            got, got_buf = _offset(np.full((B, w["det"].size), POISON, dtype=np.uint8), torch)
            step.gather(k, d_res, out=got)
            _same(_np(got), wm.gather(residual, w["det"]), what + " gather")
            _same(_np(d_res), residual, what + " gather leaves the residual alone")
            assert _untouched(got_buf, got.numel())
            win_guess = rng.integers(0, 4, size=(B, w["mech"].size), dtype=np.uint8)   # byte values 2 and 3 too
            win_conv = rng.integers(0, 3, size=B, dtype=np.uint8)
            d_wg, _ = _offset(win_guess, torch)
            d_wc, _ = _offset(win_conv, torch)
            with_next = k + 1 < K and (k + B // 2) % 2 == 0
            with_conv = (k + B) % 3 != 0
            nxt = nxt_buf = None
            if with_next:
                nxt, nxt_buf = _offset(np.full((B, windows[k + 1]["det"].size), POISON, dtype=np.uint8), torch)
            step.commit(k, d_wg, d_res, d_guess, win_conv=d_wc if with_conv else None, conv=d_conv if with_conv else None,
                        next_syndromes=nxt)
            want_next = wm.commit(H, windows, k, win_guess, residual, guess, win_conv if with_conv else None,
                                  conv if with_conv else None, want_next=with_next)
            _same(_np(d_res), residual, what + " residual (untouched bytes included)")
            _same(_np(d_guess), guess, what + " guess (untouched bytes included)")
            _same(_np(d_conv), conv, what + " flags")
            _same(_np(d_wg), win_guess, what + " the window's guess is only read")
            if with_next:
                _same(_np(nxt), want_next, what + " next window's syndromes")
                assert _untouched(nxt_buf, nxt.numel())
            assert _untouched(res_buf, residual.size) and _untouched(guess_buf, guess.size) and _untouched(conv_buf, conv.size)
        assert (guess == POISON).any() and (residual == POISON).any()          # bytes that no window owns kept the poison
    step.close()


def test_step_kernel_reads_a_long_guess_from_global_memory(ldpc, gpu):
    """A window of 1.4 million mechanisms: its bit image is beyond the LDS, the walks read the guess bytes themselves.
    The expectation is the rule in matrix form (the per-mechanism model would loop 1.4 million times)."""
    import torch

    D, N, B = 64, 1_400_000, 3
    rng = np.random.default_rng(8)
    H = sp.csc_matrix((np.ones(N, dtype=np.uint8), rng.integers(0, D - 1, size=N), np.arange(N + 1)), shape=(D, N))
    step = ldpc.WindowStep(H, [np.arange(0, D, 2), np.arange(D)], [np.arange(N), np.zeros(0, dtype=np.int64)],
                           [np.arange(0, N, 3), np.zeros(0, dtype=np.int64)])
    residual = rng.integers(0, 4, size=(B, D), dtype=np.uint8)
    win_guess = rng.integers(0, 4, size=(B, N), dtype=np.uint8)
    d_res, d_wg = torch.from_numpy(residual).cuda(), torch.from_numpy(win_guess).cuda()
    d_guess = torch.full((B, N), POISON, dtype=torch.uint8, device="cuda")
    nxt = torch.full((B, D), POISON, dtype=torch.uint8, device="cuda")
    step.commit(0, d_wg, d_res, d_guess, next_syndromes=nxt)
    kept = np.zeros(N, dtype=bool)
    kept[::3] = True
    want_guess = np.where(kept[None, :], win_guess & 1, POISON).astype(np.uint8)
    Hc = sp.csr_matrix(H[:, kept].astype(np.int64))
    flips = (Hc @ (win_guess[:, kept] & 1).T.astype(np.int64)).T & 1
    want_res = ((residual & 1) ^ flips).astype(np.uint8)
    want_res[:, D - 1] = residual[:, D - 1]                        # no column touches the last detector: not owned
    _same(_np(d_guess), want_guess, "guess")
    _same(_np(d_res), want_res, "residual")
    _same(_np(nxt), want_res & 1, "next window's syndromes")
    step.close()


def test_step_refusals_that_need_a_device(ldpc, gpu):
    import torch

    H, windows = _random_step(37, 300, 4, seed=37)
    step = ldpc.WindowStep(H, [w["det"] for w in windows], [w["mech"] for w in windows], [w["commit"] for w in windows])
    B = 5
    res = torch.full((B, 37), POISON, dtype=torch.uint8, device="cuda")
    guess = torch.full((B, 300), POISON, dtype=torch.uint8, device="cuda")
    wg = torch.zeros((B, 300), dtype=torch.uint8, device="cuda")
    out = torch.full((B, 37), POISON, dtype=torch.uint8, device="cuda")
    h, p = step._h, (lambda t: t.data_ptr())
    err = lambda: gpu.ldpc_last_error().decode()
    for k in (-1, 4):
        assert gpu.ldpc_windows_gather_device(h, k, B, p(res), p(out), None) == INVALID and f"window {k}" in err()
        assert gpu.ldpc_windows_commit_device(h, k, B, p(wg), None, p(res), p(guess), None, None, None) == INVALID and f"window {k}" in err()
    assert gpu.ldpc_windows_commit_device(h, 3, B, p(wg), None, p(res), p(guess), None, p(out), None) == INVALID and "window 3" in err()
    assert gpu.ldpc_windows_commit_device(h, 3, 0, p(wg), None, p(res), p(guess), None, p(out), None) == INVALID
    assert gpu.ldpc_windows_gather_device(h, 0, -1, p(res), p(out), None) == INVALID and "batch" in err()
    assert gpu.ldpc_windows_commit_device(h, 0, -1, p(wg), None, p(res), p(guess), None, None, None) == INVALID and "batch" in err()
    assert gpu.ldpc_windows_gather_device(h, 0, B, None, p(out), None) == INVALID and "window 0" in err() and "residual" in err()
    assert gpu.ldpc_windows_gather_device(h, 0, B, p(res), None, None) == INVALID and "syndromes" in err()
    assert gpu.ldpc_windows_commit_device(h, 1, B, None, None, p(res), p(guess), None, None, None) == INVALID and "window 1" in err()
    assert gpu.ldpc_windows_commit_device(h, 1, B, p(wg), None, None, p(guess), None, None, None) == INVALID and "residual" in err()
    assert gpu.ldpc_windows_commit_device(h, 1, B, p(wg), None, p(res), None, None, None, None) == INVALID and "guess" in err()
    # batch 0: LDPC_OK, nothing touched (not even looked at)
    assert gpu.ldpc_windows_gather_device(h, 0, 0, None, None, None) == 0
    assert gpu.ldpc_windows_commit_device(h, 0, 0, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    for t in (res, guess, out):
        assert bool((t == POISON).all())
    # a bad list is refused with a device as without one
    bad = [w["det"].copy() for w in windows]
    bad[2][1] = bad[2][0]
    with pytest.raises(ldpc.LdpcError) as ei:
        ldpc.WindowStep(H, bad, [w["mech"] for w in windows], [w["commit"] for w in windows])
    assert ei.value.status == INVALID and "window 2: det_idx[1]" in ei.value.message
    step.close()


# ---- the decoder: the BB-72 fixture ------------------------------------------------------------------------------------

TRIALS = 300                    # the run_dem_trials test; its first 200 columns are the fixture's syndromes
LEGS = [4, 3, 3]


def _minsum_of(H, rates):
    model = MinSumModel(H, llr_of_probs(rates), 30)
    return lambda s: model.decode(s)[:2]


def _gammas(n):
    g = np.empty((3, n), dtype=np.float32)
    g[0] = 0.125
    g[1:] = np.random.default_rng(5).uniform(-0.24, 0.66, size=(2, n)).astype(np.float32)
    return g


@pytest.fixture(scope="module")
def fixture(ldpc):
    """phenomenological(HX, logicals, 5, 0.01, 0.02) of BB-72, W = 3, C = 1, the model's errors and syndromes of seed 7
    and the model chain around min-sum on all of them, computed once."""
    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    logicals = ldpc.codes.css_logicals(HX, HZ)[1]
    dem = ldpc.phenomenological(HX, logicals, 5, 0.01, 0.02)
    errors = dm.sample(dem.rates, TRIALS, 7, 0)
    syn = tm.syndromes(dem.H, errors)
    layers = ldpc.phenomenological_layers(HX, 5)
    windows, uncovered = wm.plan(dem.H, layers, 3, 1)
    chain = wm.chain(dem.H, dem.rates, windows, uncovered, _minsum_of, syn)[:3]
    for a in (errors, syn) + chain:
        a.setflags(write=False)
    return SimpleFixture(HX=HX, logicals=logicals, dem=dem, errors=errors, syn=syn, layers=layers, windows=windows,
                         uncovered=uncovered, chain=chain)


class SimpleFixture:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _check_decoder(dec, syn, want, what):
    guess, conv, residual = dec.decode_batch_host(syn)
    _same(guess, want[0], what + " errors")
    _same(conv, want[1], what + " flags")
    _same(residual, want[2], what + " residual")
    _same(_np(dec.residual), want[2], what + " .residual")


def test_min_sum_windows_equal_the_model_chain(ldpc, gpu, fixture):
    f = fixture
    made = []

    def make(m):
        made.append(m)
        return ldpc.MinSumDecoder(m.H, None, 30, channel_probs=m.rates)
    dec = ldpc.SlidingWindowDecoder(f.dem, f.layers, 3, 1, make)
    assert len(made) == 2 and len(dec.decoders) == 2 and dec.window_decoder == [0, 0, 1] and len(dec.plan) == 3
    assert dec.sparse_H is f.dem.H and dec.per is None and dec.info().device == 0
    syn, want = f.syn[:200], tuple(a[:200] for a in f.chain)
    _check_decoder(dec, syn, want, "min-sum")
    assert 0 < int(want[1].sum()) < 200 and int(want[2].any(axis=1).sum()) > 0
    _same(want[2], syn ^ tm.syndromes(f.dem.H, want[0]), "the identity of the model chain")
    # a smaller and a larger batch on the same handle (the buffers are kept, then regrown), and the generic entries
    _check_decoder(dec, syn[:7], tuple(a[:7] for a in want), "min-sum, 7 columns")
    _check_decoder(dec, f.syn, f.chain, "min-sum, 300 columns")
    errors = np.zeros((f.dem.num_mechanisms, 5), dtype=np.uint8)
    _, success = ldpc.batchdecode_(dec, syn[:5].T, errors)
    _same(errors.T, want[0][:5], "batchdecode_")
    _same(success, want[1][:5].astype(bool), "batchdecode_ success")
    guess, ok = dec.decode_(syn[3])
    _same(guess, want[0][3].astype(np.float64), "decode_")
    assert ok == bool(want[1][3])
    dec.close()


def test_min_sum_windows_on_a_side_stream(ldpc, gpu, fixture):
    import torch

    f = fixture
    dec = ldpc.SlidingWindowDecoder(f.dem, f.layers, 3, 1, lambda m: ldpc.MinSumDecoder(m.H, None, 30, channel_probs=m.rates))
    side = torch.cuda.Stream()
    syn = torch.from_numpy(f.syn[:67].copy()).cuda()
    err = torch.full((67, f.dem.num_mechanisms), POISON, dtype=torch.uint8, device="cuda")
    conv = torch.full((67,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(syn, err, conv, stream=side.cuda_stream)
    side.synchronize()
    _same(_np(err), f.chain[0][:67], "errors")
    _same(_np(conv), f.chain[1][:67], "flags")
    _same(_np(dec.residual), f.chain[2][:67], "residual")
    dec.close()


def test_relay_windows_equal_the_model_chain(ldpc, gpu, fixture):
    f = fixture
    syn = f.syn[:200]

    def relay_of(H, rates):
        model = RelayModel(H, llr_of_probs(rates), _gammas(H.shape[1]), LEGS)
        return lambda s: model.decode(s)[:2]
    want = wm.chain(f.dem.H, f.dem.rates, f.windows, f.uncovered, relay_of, syn)[:3]
    dec = ldpc.SlidingWindowDecoder(f.dem, f.layers, 3, 1, lambda m: ldpc.RelayMinSumDecoder(
        m.H, None, LEGS[0], channel_probs=m.rates, legs=3, leg_iters=LEGS[1], gammas=_gammas(m.num_mechanisms)))
    _check_decoder(dec, syn, want, "relay")
    assert 0 < int(want[1].sum()) < 200
    dec.close()


def test_two_windows_and_one_window(ldpc, gpu, fixture):
    """(R, W, C) = (6, 4, 2): two windows, against the model chain.  width >= R: one window, the model itself -- what
    MinSumDecoder(dem.H, ...) returns on the GPU, in every element."""
    import torch

    f = fixture
    dem = ldpc.phenomenological(f.HX, f.logicals, 6, 0.01, 0.02)
    layers = ldpc.phenomenological_layers(f.HX, 6)
    syn = tm.syndromes(dem.H, dm.sample(dem.rates, 100, 11, 0))
    make = lambda m: ldpc.MinSumDecoder(m.H, None, 30, channel_probs=m.rates)
    windows, uncovered = wm.plan(dem.H, layers, 4, 2)
    assert len(windows) == 2
    dec = ldpc.SlidingWindowDecoder(dem, layers, 4, 2, make)
    assert dec.window_decoder == [0, 1]
    _check_decoder(dec, syn, wm.chain(dem.H, dem.rates, windows, uncovered, _minsum_of, syn)[:3], "(6, 4, 2)")
    dec.close()
    one_shot = make(dem)
    want_err, want_conv, _, _ = one_shot.decode_batch_host(syn)
    one_shot.close()
    for W, C in ((6, 1), (9, 4)):
        dec = ldpc.SlidingWindowDecoder(dem, layers, W, C, make)
        assert len(dec.plan) == 1 and dec.plan.sub_model(0) == ldpc.DetectorErrorModel(dem.H, None, dem.rates)
        guess, conv, residual = dec.decode_batch_host(syn)
        _same(guess, want_err, f"width {W}: errors against the one-shot decoder")
        _same(conv, want_conv, f"width {W}: flags against the one-shot decoder")
        _same(residual, syn ^ tm.syndromes(dem.H, want_err), f"width {W}: residual")
        dec.close()


def test_run_dem_trials_drives_the_window_decoder(ldpc, gpu, fixture):
    f = fixture
    dec = ldpc.SlidingWindowDecoder(f.dem, f.layers, 3, 1, lambda m: ldpc.MinSumDecoder(m.H, None, 30, channel_probs=m.rates))
    res = ldpc.run_dem_trials(f.dem, dec, TRIALS, batch=128, seed=7)           # 128 + 128 + 44: a ragged last batch
    _, c = tm.score(f.dem.H, f.dem.L, f.chain[0], f.errors)
    want = (int(c[0]), int(c[1]), int(c[2]), int(c[3]), int((f.chain[1] == 0).sum()))
    print("sliding-window min-sum:", res)
    assert (res.trials, res.block_errors, res.syndrome_mismatches, res.logical_errors, res.not_converged) == want
    assert want[0] == TRIALS and 0 < res.block_errors < TRIALS and res.not_converged > 0
    dec.close()
    with pytest.raises(ValueError):                                            # another model's decoder
        other = ldpc.phenomenological(f.HX, f.logicals, 4, 0.01, 0.02)
        ldpc.run_dem_trials(other, dec, 10)


def test_bp_windows_equal_the_oracle_chain(ldpc, gpu, fixture):
    """BeliefPropagationDecoder per window at p = q = 0.01 (one prior for all bits is then the model's own)."""
    from oracle import BPOracle

    f = fixture
    dem = ldpc.phenomenological(f.HX, f.logicals, 5, 0.01, 0.01)
    syn = tm.syndromes(dem.H, dm.sample(dem.rates, 200, 7, 0))

    def oracle_of(H, rates):
        assert np.all(rates == 0.01)
        H = sp.csc_matrix(H)
        H.sort_indices()
        oc = BPOracle(csc=(H.indptr, H.indices), shape=H.shape, per=0.01, max_iters=20)
        return lambda s: oc.batchdecode(s, want_llr=False)[:2]
    want = wm.chain(dem.H, dem.rates, f.windows, f.uncovered, oracle_of, syn)[:3]
    dec = ldpc.SlidingWindowDecoder(dem, f.layers, 3, 1, lambda m: ldpc.BeliefPropagationDecoder(m.H, 0.01, 20))
    _check_decoder(dec, syn, want, "BP")
    assert 0 < int(want[1].sum()) < 200
    dec.close()


def test_bposd_windows_equal_the_model_chain(ldpc, gpu, fixture):
    """BeliefPropagationOSDDecoder(bp_decoder=MinSumDecoder, osd="device") as the window decoder: a converged column keeps
    its min-sum guess (osd_order 0), any other gets the ordered-statistics step -- so every window's guess reproduces
    its window's syndromes wherever they are consistent."""
    f = fixture
    syn = f.syn[:60]

    def bposd_of(H, rates):
        model = MinSumModel(H, llr_of_probs(rates), 30)
        Hd = np.asarray(sp.csc_matrix(H).todense()).astype(np.uint8)

        def decode(s):
            err, conv, _, L = model.decode(s)
            out = np.stack([err[b] if conv[b] else osd_model_postprocess(Hd, s[b], err[b], L[b].astype(np.float64), 0)
                            for b in range(s.shape[0])])
            return out, conv
        return decode
    want = wm.chain(f.dem.H, f.dem.rates, f.windows, f.uncovered, bposd_of, syn)[:3]
    made = []

    def make(m):
        made.append(ldpc.MinSumDecoder(m.H, None, 30, channel_probs=m.rates))
        return ldpc.BeliefPropagationOSDDecoder(m.H, osd_order=0, osd="device", bp_decoder=made[-1])
    dec = ldpc.SlidingWindowDecoder(f.dem, f.layers, 3, 1, make)
    guess, conv, residual = dec.decode_batch_host(syn)
    _same(residual, syn ^ tm.syndromes(f.dem.H, guess), "residual == syn ^ H guess")
    _same(guess, want[0], "BP+OSD errors")
    _same(conv, want[1], "BP+OSD flags")
    _same(residual, want[2], "BP+OSD residual")
    assert int((want[1] == 0).sum()) > 0 and int((want[0] != f.chain[0][:60]).any(axis=1).sum()) > 0   # the OSD step changed a guess
    dec.close()
    for d in made:
        d.close()
