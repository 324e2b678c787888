"""The standard rule of the OSD step on the GPU (ldpc_osd_set_search + ldpc_osd_postprocess_batch_device;
csrc/osd_search_kernels.hpp) against its numpy model (tests/osd_search_model.py), fed the same syn, bp_err and llr the
device read.  The rule is integer arithmetic and exact comparisons: equality in every element of every syndrome.  Every
syndrome is built as H e, so none lies outside the column space."""
import numpy as np
import pytest
import scipy.sparse as sp

from osd_search_model import METHODS, osd_search_model, weights_of

pytestmark = pytest.mark.gpu


def _dense(H):
    return np.asarray(sp.csc_matrix(H).todense()).astype(np.uint8)


def _syn_of(Hd, e):
    return ((e.astype(np.int64) @ Hd.T.astype(np.int64)) % 2).astype(np.uint8)


def _state_bytes(m, n):
    """osd_search_state_bytes, as include/ldpc_mi355x.h states it."""
    up = lambda v: (v + 15) & ~15
    nw, mw = (n + 63) >> 6, (m + 63) >> 6
    st = (nw + 1) | 1
    return up(m * st * 8) + up(8 * n) + 2 * up(4 * n) + up(4 * m) + up(8 * m) + 2 * up((nw + 1) * 8) + up(65 * (mw + 1) * 8)


def _device(ldpc, H, method, order, syn, err, llr, weights=None, variant=0, tier=None, inplace=False, post=None):
    import torch

    own = post is None
    if own:
        post = ldpc.OSDPostProcessor(H, order, method=method, weights=weights)
        post.prepare_device(0, variant)
    if tier is not None:
        assert post.kernel == tier, (post.kernel, tier)
    d_syn = torch.from_numpy(np.array(syn, dtype=np.uint8)).to("cuda:0")
    d_err = torch.from_numpy(np.array(err, dtype=np.uint8)).to("cuda:0")
    d_llr = torch.from_numpy(np.array(llr, dtype=np.float64)).to("cuda:0")
    out = post.postprocess_device(d_syn, d_err, d_llr, out=d_err if inplace else None)
    torch.cuda.synchronize()
    if not inplace:
        assert np.array_equal(d_err.cpu().numpy(), err), "bp_errors was written by an out-of-place call"
    res = out.cpu().numpy()
    if own:
        post.close()
    return res


def _model(Hd, method, order, syn, err, llr, weights=None):
    q = None if weights is None else weights_of(weights)
    return np.array([osd_search_model(Hd, syn[b], err[b], llr[b], METHODS[method], order, q) for b in range(syn.shape[0])],
                    dtype=np.uint8).reshape(syn.shape[0], Hd.shape[1])


def _against_model(ldpc, H, method, order, syn, err, llr, weights=None, variants=(0,), ref=None, **kw):
    Hd = _dense(H)
    if ref is None:
        ref = _model(Hd, method, order, syn, err, llr, weights)
    assert np.array_equal(_syn_of(Hd, ref), (syn != 0).astype(np.uint8)), "a model output does not reproduce its syndrome"
    for variant in variants:
        out = _device(ldpc, H, method, order, syn, err, llr, weights=weights, variant=variant, **kw)
        bad = np.nonzero((out != ref).any(axis=1))[0]
        assert bad.size == 0, f"{method} order {order} variant {variant}: the kernel differs from the model on syndromes {bad[:8]}"
    return ref


def _random_inputs(rng, Hd, B, ties=0.3):
    """Drawn, not decoded: any bp_err / llr row is a valid input; the syndromes are those of random errors."""
    n = Hd.shape[1]
    E = (rng.random((B, n)) < 0.08).astype(np.uint8)
    err = (rng.random((B, n)) < 0.05).astype(np.uint8)
    llr = rng.normal(1.0, 3.0, (B, n))
    llr[rng.random((B, n)) < ties] = 0.75
    return _syn_of(Hd, E), err, llr


_BB = {}
PER = 0.06


def _bb72(ldpc):
    """BB-72 H_X (36 x 72, rank 30: six unused rows; K = 42).  200 syndromes of errors at 0.06 with the GPU min-sum
    decoder's own hard decisions and LLRs -- 150 it leaves unconverged and 50 it converges on -- and 100 drawn inputs."""
    if not _BB:
        HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
        H = sp.csc_matrix(HX)
        Hd = _dense(H)
        syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 3000, PER, seed=3))
        dec = ldpc.MinSumDecoder(H, PER, 30)
        err, conv, llr = dec.decode_batch_host(syn, want_llr=True)[:3]
        prior = np.asarray(dec.channel_llr, dtype=np.float64)
        dec.close()
        pick = np.concatenate([np.nonzero(conv == 0)[0][:150], np.nonzero(conv == 1)[0][:50]])
        assert pick.size == 200
        s2, e2, l2 = _random_inputs(np.random.default_rng(1), Hd, 100)
        _BB["case"] = (H, Hd, np.concatenate([syn[pick], s2]), np.concatenate([err[pick], e2]),
                       np.concatenate([np.asarray(llr[pick], dtype=np.float64), l2]), prior)
        for a in _BB["case"][2:]:
            a.setflags(write=False)
    return _BB["case"]


def _prior_weights(n=72):
    """Two rates, as a model with data and measurement errors has them."""
    p = np.where(np.arange(n) % 3 == 0, 0.02, PER)
    return np.log((1 - p) / p)


@pytest.mark.parametrize("weights", ["hamming", "priors"])
@pytest.mark.parametrize("method,order", [("combination_sweep", o) for o in (0, 1, 2, 10, 16, 64)] +
                         [("exhaustive", o) for o in (0, 1, 2, 10, 16)])
def test_bb72_every_order_every_tier(ldpc, gpu, method, order, weights):
    """lambda = 64 > K = 42 is clamped by the sweep.  Orders 10 and 16 of the exhaustive search on fewer syndromes: the
    model enumerates 2^order candidates."""
    H, Hd, syn, err, llr, _ = _bb72(ldpc)
    cut = slice(120, 180) if (method == "exhaustive" and order >= 10) else slice(None)
    w = None if weights == "hamming" else _prior_weights()
    for variant in (1, 2, 3):
        ref = _against_model(ldpc, H, method, order, syn[cut], err[cut], llr[cut], weights=w, variants=(variant,), tier=variant,
                             ref=None if variant == 1 else ref)
    assert (ref != err[cut]).any()


@pytest.mark.parametrize("n", [63, 64, 65])
def test_one_row_and_word_boundaries(ldpc, gpu, n):
    rng = np.random.default_rng(n)
    Hd = (rng.random((1, n)) < 0.5).astype(np.uint8)
    Hd[0, n - 1] = 1
    syn, err, llr = _random_inputs(rng, Hd, 60)
    for method, order in (("combination_sweep", 0), ("combination_sweep", 64), ("exhaustive", 5)):
        _against_model(ldpc, sp.csc_matrix(Hd), method, order, syn, err, llr, variants=(0, 2, 3), weights=rng.normal(0, 2, n))


def test_identity_has_one_candidate(ldpc, gpu):
    """K = 0: only candidate 0, whatever the method and the order; the output is the syndrome itself."""
    rng = np.random.default_rng(4)
    Hd = np.eye(20, dtype=np.uint8)
    syn, err, llr = _random_inputs(rng, Hd, 30)
    for method, order in (("combination_sweep", 10), ("exhaustive", 16), ("exhaustive", 0)):
        ref = _against_model(ldpc, sp.csc_matrix(Hd), method, order, syn, err, llr, variants=(0, 2, 3))
        assert np.array_equal(ref, syn)


def test_a_thread_owns_two_rows(ldpc, gpu):
    """1100 rows for the 1024 threads of a workgroup (128 columns: the state, 51 KiB, fits tier 2)."""
    rng = np.random.default_rng(6)
    Hd = (rng.random((1100, 128)) < 0.04).astype(np.uint8)
    syn, err, llr = _random_inputs(rng, Hd, 12)
    assert _state_bytes(1100, 128) <= 159 * 1024
    for method, order in (("combination_sweep", 10), ("exhaustive", 4)):
        _against_model(ldpc, sp.csc_matrix(Hd), method, order, syn, err, llr, tier=2, weights=rng.uniform(0.5, 4, 128))
        _against_model(ldpc, sp.csc_matrix(Hd), method, order, syn, err, llr, variants=(3,), tier=3)


@pytest.mark.parametrize("s,n,tier", [(128, 512, 1), (129, 512, 2), (128, 513, 2), (933, 1000, 2), (934, 1000, 3)])
def test_shapes_at_the_tier_bounds(ldpc, gpu, s, n, tier):
    """Tier 1 up to 128 x 512; tier 2 up to 159 KiB of state: 933 x 1000 is 96 bytes under, 934 x 1000 is 32 over."""
    assert (s <= 128 and n <= 512) == (tier == 1) and (_state_bytes(s, n) <= 159 * 1024) == (tier <= 2)
    rng = np.random.default_rng(s + n)
    Hd = (rng.random((s, n)) < 6.0 / s).astype(np.uint8)
    syn, err, llr = _random_inputs(rng, Hd, 6 if tier == 1 else 3)
    _against_model(ldpc, sp.csc_matrix(Hd), "combination_sweep", 10, syn, err, llr, tier=tier, weights=rng.uniform(0.5, 4, n))
    _against_model(ldpc, sp.csc_matrix(Hd), "exhaustive", 3, syn, err, llr, tier=tier)


def test_llr_edge_inputs(ldpc, gpu):
    """All equal (order by index alone), +-0.0 mixed, +-inf, NaNs (last, by index), and a mix of all of them."""
    H, Hd, syn, err, llr, _ = _bb72(ldpc)
    rng = np.random.default_rng(8)
    syn, err = syn[:60], err[:60]
    rows = np.array(llr[:60])
    rows[0:10] = 1.25
    rows[10:20] = np.where(rng.random((10, 72)) < 0.5, 0.0, -0.0)
    rows[20:30] = rng.choice([-np.inf, np.inf, -1.0, 2.0], size=(10, 72))
    rows[30:40][rng.random((10, 72)) < 0.4] = np.nan
    rows[40] = np.nan
    rows[41] = np.inf
    rows[42] = -np.inf
    rows[43:60] = rng.choice([np.nan, -np.inf, np.inf, 0.0, -0.0, -3.5, 3.5, 5e-324, -5e-324], size=(17, 72))
    for method, order in (("combination_sweep", 10), ("exhaustive", 3)):
        _against_model(ldpc, H, method, order, syn, err, rows, variants=(1, 2, 3))
        _against_model(ldpc, H, method, order, syn, err, rows, variants=(1, 3), weights=_prior_weights())


def test_weights_equal_negative_and_beyond_32_bits(ldpc, gpu):
    H, Hd, syn, err, llr, _ = _bb72(ldpc)
    rng = np.random.default_rng(9)
    syn, err, llr = syn[:150], err[:150], llr[:150]
    zero = np.zeros(72)                                   # every candidate costs 0: index 0 wins
    ref = _against_model(ldpc, H, "combination_sweep", 10, syn, err, llr, weights=zero, variants=(1, 3))
    assert np.array_equal(ref, _model(Hd, "exhaustive", 0, syn, err, llr))
    _against_model(ldpc, H, "exhaustive", 6, syn, err, llr, weights=zero, variants=(1, 2))
    negative = rng.uniform(-3, 3, 72)
    clamp = rng.choice([1e9, 2.0 ** 24, 1.0, 2.0 ** -16, -2.0 ** 24, -1e9], size=72)    # costs of several 2^40, and differences of 1
    assert np.abs(weights_of(clamp)).max() == 2 ** 40
    for w in (negative, clamp):
        _against_model(ldpc, H, "combination_sweep", 10, syn, err, llr, weights=w, variants=(1, 2, 3))
        _against_model(ldpc, H, "exhaustive", 8, syn[:60], err[:60], llr[:60], weights=w, variants=(1, 3))


def test_bp_estimate_that_reproduces_the_syndrome_is_returned_unchanged(ldpc, gpu):
    """Step 1 at lambda = 10: an estimate heavier than the error by two stabiliser rows is not the lightest solution."""
    H, Hd, _, _, llr, _ = _bb72(ldpc)
    rng = np.random.default_rng(10)
    E = (rng.random((80, 72)) < 0.04).astype(np.uint8)
    syn = _syn_of(Hd, E)
    HZ = _dense(ldpc.codes.bivariate_bicycle_72_12_6()[1])
    heavy = E ^ HZ[rng.integers(0, 36, 80)] ^ HZ[rng.integers(0, 36, 80)]
    assert np.array_equal(_syn_of(Hd, heavy), syn) and heavy.sum() > E.sum() + 80
    for method in ("combination_sweep", "exhaustive"):
        for w in (None, _prior_weights()):
            for variant in (1, 2, 3):
                out = _device(ldpc, H, method, 10, syn, heavy, llr[:80], weights=w, variant=variant)
                assert np.array_equal(out, heavy)
    assert np.array_equal(_model(Hd, "combination_sweep", 10, syn, heavy, llr[:80]), heavy)


def test_launch_cases(ldpc, gpu):
    """In place; a handle used three times; a batch of 1; a batch beyond the grid (1200 syndromes for the at most 512
    workgroups of 1024 threads that a device of 256 CUs holds); two streams on one tier-3 handle."""
    import torch

    H, Hd, syn, err, llr, _ = _bb72(ldpc)
    syn, err, llr = np.tile(syn, (4, 1)), np.tile(err, (4, 1)), np.tile(llr, (4, 1))
    w = _prior_weights()
    ref = np.tile(_model(Hd, "combination_sweep", 10, syn[:300], err[:300], llr[:300], w), (4, 1))
    for variant in (2, 3):
        post = ldpc.OSDPostProcessor(H, 10, method="combination_sweep", weights=w)
        assert post.prepare_device(0, variant) == variant
        a = _device(ldpc, H, "combination_sweep", 10, syn, err, llr, post=post)
        b = _device(ldpc, H, "combination_sweep", 10, syn, err, llr, post=post, inplace=True)
        c = _device(ldpc, H, "combination_sweep", 10, syn[7:8], err[7:8], llr[7:8], post=post)
        assert np.array_equal(a, ref) and np.array_equal(b, ref) and np.array_equal(c, ref[7:8])
        d_syn, d_err, d_llr = (torch.from_numpy(x.copy()).to("cuda:0") for x in (syn, err, llr))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s1):
            o1 = post.postprocess_device(d_syn, d_err, d_llr)
        with torch.cuda.stream(s2):
            o2 = post.postprocess_device(d_syn[:700].contiguous(), d_err[:700].contiguous(), d_llr[:700].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(o1.cpu().numpy(), ref) and np.array_equal(o2.cpu().numpy(), ref[:700])
        post.close()


def test_end_to_end_decoder_and_dem_trials(ldpc, gpu):
    """BeliefPropagationOSDDecoder on a MinSumDecoder, CS-10 with prior weights: batchdecode_device equals the model
    applied to the min-sum MODEL's outputs, only the unconverged syndromes are sent; the host-array entries go through
    the same kernel; run_dem_trials drives the same construction on a phenomenological BB-72 model of two rounds."""
    import torch
    from minsum_model import MinSumModel, llr_of_probs

    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    H = sp.csc_matrix(HX)
    Hd = _dense(H)
    probs = np.where(np.arange(72) % 3 == 0, 0.02, PER)
    B = 1500
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, B, PER, seed=5))
    merr, mconv, _, mL = MinSumModel(H, llr_of_probs(probs), 30).decode(syn)
    ms = ldpc.MinSumDecoder(H, channel_probs=probs, max_iters=30)
    dec = ldpc.BeliefPropagationOSDDecoder(HX, bp_decoder=ms, osd="device", osd_method="combination_sweep", osd_order=10,
                                           osd_weights="priors")
    assert dec._osd.kernel == 1 and dec._osd._L.ldpc_osd_search_method(dec._osd._h) == 2
    q = weights_of(np.asarray(ms.channel_llr, dtype=np.float64))
    assert [int(dec._osd._L.ldpc_osd_search_weight(dec._osd._h, j)) for j in range(72)] == q.tolist()
    for call in range(2):
        gerr, gconv, sent = dec.batchdecode_device(torch.from_numpy(syn).to("cuda:0"))
        torch.cuda.synchronize()
        gerr, gconv = gerr.cpu().numpy(), gconv.cpu().numpy()
        assert np.array_equal(gconv, mconv) and sent == int((mconv == 0).sum()) and 0 < sent < B
        for b in range(B):
            want = merr[b] if mconv[b] else osd_search_model(Hd, syn[b], merr[b], np.asarray(mL[b], dtype=np.float64), 2, 10, q)
            assert np.array_equal(gerr[b], want), f"syndrome {b} differs from the model chain"
    assert np.array_equal(_syn_of(Hd, gerr), syn)
    out = np.zeros((72, 300), dtype=np.uint8)
    g, c = dec.batchdecode_(syn[:300].T, out)
    assert np.array_equal(g.T, gerr[:300]) and np.array_equal(c, gconv[:300].astype(bool))
    g1, c1 = dec.decode_(syn[11])
    assert np.array_equal(g1.astype(np.uint8), gerr[11]) and c1 == bool(gconv[11])
    # a detector error model: data errors at 0.03, measurement errors at 0.05
    dem = ldpc.phenomenological(HX, ldpc.codes.css_logicals(HX, HZ)[1], 2, 0.03, 0.05)
    ms2 = ldpc.MinSumDecoder(dem.H, channel_probs=dem.rates, max_iters=30)
    plain = ldpc.run_dem_trials(dem, ms2, 4000, batch=1024, seed=2)
    osd = ldpc.BeliefPropagationOSDDecoder(dem.H, bp_decoder=ms2, osd="device", osd_method="combination_sweep", osd_order=10,
                                           osd_weights="priors")
    res = ldpc.run_dem_trials(dem, osd, 4000, batch=1024, seed=2)
    print(f"phenomenological BB-72, R = 2, 4000 trials: min-sum(30) {plain.block_errors} block errors ({plain.syndrome_mismatches} miss "
          f"the syndrome); + CS-10 with prior weights {res.block_errors} ({res.syndrome_mismatches})")
    assert res.trials == plain.trials == 4000
    assert plain.syndrome_mismatches > 0 and res.syndrome_mismatches == 0   # every syndrome is H e: OSD reproduces all of them
